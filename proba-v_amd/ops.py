"""torch custom ops (`torch.ops.probav.*`) over the C ABI of libprobav_hip.so -- the north-star boundary: the hot path is
"hand-written HIP kernels exposed as torch custom ops"; PyTorch owns device memory, the stream and the autograd graph, nothing else.

Registered with `torch.library.custom_op` (schema, dispatcher entry, fake-tensor rule, autograd formula), so they are visible to the
dispatcher, `torch.compile` / AOT-autograd and `torch.library.opcheck` (tests/test_gpu_ops.py):

  probav::wdsr_forward(flat, x, engine, out_size, training) -> (y, ws)      model(x, training=...)      models/trainClass.py:127,139
  probav::wdsr_backward(flat, dy, ws, engine) -> dflat                      tape.gradient(loss, vars)   models/trainClass.py:131
  probav::wdsr_backward_input(flat, dy, ws, engine) -> (dflat, dx)          tape.gradient(loss, [x] + vars): called instead of wdsr_backward
                                                                            when the model input requires grad (modelsTF.py:23-27, 45-53, 58 in reverse)
  probav::shift_loss(pred, hr, mask, border, bit_depth, which) -> (loss, arg, per_sample)
                                                                            Losses.shiftCompensatedL1Loss / L2Loss   models/loss.py:55-84
  probav::shift_loss_backward(hr, mask, pred, arg, upstream, border, which) -> dpred
  probav::shift_metrics(hr, mask, pred, border, bit_depth) -> (f[3,B], arg[2,B], means[2])     one launch: L1, L2, cPSNR of every sample
  probav::shift_l1edge_loss(pred, hr, mask, border, pi) -> (loss, arg [B], per_sample [B])   Losses.shiftCompensatedL1EdgeLoss (cfg sobel_l1_mix)   models/loss.py:86-97
  probav::shift_l1edge_loss_backward(hr, mask, pred, arg, upstream, border, pi) -> dpred
  probav::revssim_loss(pred, hr, mask, border, bit_depth, eta) -> (loss, arg [1], moments f64 [shifts, B, 5, 7])
                                                                            Losses.shiftCompensatedRevSSIM (cfg l1msssim)   models/loss.py:99-124
  probav::revssim_loss_backward(hr, mask, pred, arg, moments, upstream, border, bit_depth, eta) -> dpred
  probav::nadam_step(theta, grad, m, v, lr, b1, b2, eps, c_g, c_m, c_v) -> ()                 optimizer.apply_gradients   trainClass.py:132
  probav::optimizer_wn_step(theta, grad, m, v, wcache, engine, lr, ...) -> ()                 the same update fused with the weight normalisation
                                                                            and operand packing of the NEXT step (wdsr_forward's optional `wcache`)
  probav::grad_guard(grad, ctl, scratch, clipnorm, skip_nonfinite) -> ()                     tf.clip_by_global_norm's norm + the non-finite guard: the step's
                                                                            control block {scale, skip, skipped_total, norm}, on the device
  probav::nadam_step_guarded(theta, grad, m, v, ema?, ctl?, lr, ..., ema_momentum) -> ()      nadam_step with Keras global_clipnorm / use_ema + the guard
  probav::optimizer_wn_step_guarded(theta, grad, m, v, wcache, ema?, ctl?, engine, ...) -> () optimizer_wn_step with the same
  probav::clip_round(x, lo, hi) -> y                                        tf.clip_by_value + tf.round   test.py:118-119
  probav::esa_shift_moments(sr, hr, mask, border) -> moments int64 [N, (2b+1)^2, 3]       (n, s1, s2) of every shift, exact
  probav::esa_shift_cpsnr(sr, hr, mask, border) -> (cpsnr f64[N], shift i32[N,2], bias f64[N], n_clear i64[N])
                                                                            the ESA cPSNR of whole images   evaluate.py:76-87 (scoring.py)
  probav::esa_shift_ssim_table(sr, hr, mask, border) -> table f64 [N, (2b+1)^2]           the windowed SSIM of every shift, NaN where n = 0
  probav::esa_shift_cssim(sr, hr, mask, border) -> (cssim f64[N], shift i32[N,2])         its first maximum: the cSSIM published beside the cPSNR
  probav::augment_batch(lr, hr, mask, recipe) -> (lr_b, hr_b, mask_b)      a training batch from the un-augmented patches: frame permutation,
                                                                            flip, quarter turns per sample   utils/dataGenerator.py:227-273 (augment.py)
  probav::ensemble_expand(lr, recipe) -> lr_v                              the LR variants of inference patches (flip, quarter turns, frame order)
  probav::ensemble_reduce(sr, recipe, V, lo, hi, final_round, sets, grid) -> patches [N, S, S] | images [sets, grid S, grid S]
                                                                            the mean of the V clipped, rounded predictions of every patch, each turned
                                                                            back, optionally stitched   test.py:137-146, 149-160 (ensemble.py)
  probav::tile_blend(sr, w, n_images, n, hr_stride, lo, hi) -> images [n_images, G, G]
                                                                            overlapping tile predictions blended by an integer window, exact
                                                                            64-bit arithmetic, rounded half to even   test.py:149-160 (tiles.py)
  probav::frame_windows_gather(patches, counts, k, limit, windows, step, mode) -> (x [N, W, win, win, k, 1], weight [N, W], sel [N, W, k])
                                                                            the frames of every tile chosen and ordered on the device, the inputs
                                                                            of W sliding windows over them written from one read of the tile
  probav::frame_windows_reduce(sr, weight, lo, hi) -> [N, S, S]             the weighted mean of the W clipped, rounded predictions of every tile,
                                                                            exact 64-bit arithmetic, rounded half to even   (frame_windows.py)
  probav::baseline_upscale_mean(frames, clear, set_offsets, mode) -> (out [S, 3H, 3W], k_used [S])
                                                                            the competition's bicubic-mean baseline of ragged image sets, exact
                                                                            integer arithmetic   evaluate.py:142-197 (baseline.py)
  probav::window_counts(masks, pad, win, stride) -> counts int32 [M, ny, nx]  the masked pixels of every window of reflect-padded masks, exact:
                                                                            the validity table of every crop origin   (crops.py)
  probav::crop_batch(lr, lr_mask, hr, hr_clear, positions, recipe, P, pad, win, scale, limit) -> (lr_b, hr_b, mask_b, sel [B, k])
                                                                            a training batch cut at arbitrary origins out of resident scenes: the
                                                                            window's frames chosen as the builder chooses them, then frame order,
                                                                            flip, quarter turns   utils/dataGenerator.py:99-174, 326-551 (crops.py)
  probav::fusenet_forward(x, flat, residual) -> (out [B, H, W], y [B, H, W, 64], stats [B, 64, 2])
                                                                            FuseNetConv2D: 48 x 48 convolution, instance normalisation, LeakyReLU,
                                                                            channel mean, + x   models/modelsTF.py:391-474 (fusenet_numpy.py)
  probav::fusenet_backward(g, x, y, stats, flat) -> dflat                   its parameter gradients (the bias part exact zeros; no input gradient)

`engine` is the probav_engine* of include/probav_hip.h as an integer (the ops are stateless; the handle owns only the layer table),
`ws` the workspace of one forward call: an OUTPUT of wdsr_forward (it carries the activations to the reverse pass, like the residuals of
any differentiable op; torch's caching allocator recycles the block from step to step), an input of wdsr_backward.  Every op raises on CPU tensors:
there is no fallback implementation.

What an op accepts (one contract for every op; INTEGRATION.md, 'Custom ops: what an op accepts'; the cases: tests/ops_contract.py).  Each op has ONE
validator, shared by its real implementation and its fake rule, that runs before any compute entry point of the library:

  1 device     every tensor operand on one HIP device, else RuntimeError "... (no CPU fallback)" naming op and operand (a fake rule sees only
               that the operands agree)
  2 dtype      one accepted dtype per operand (bool for a uint8 mask; int16 bits for uint16 in the scoring and baseline ops), else ValueError
               naming op, operand and dtype; no operand is cast (the .float() of the autograd formulas on incoming gradients stays)
  3 read       any strides: the op reads a contiguous copy -- the bits of a fresh .contiguous() clone, the input untouched, contiguous outputs
  4 written    theta, m, v, wcache, ema, ctl, scratch: contiguous and on a 16-byte boundary, else ValueError and nothing changes
  5 offset     a contiguous view off a 16-byte boundary: copied, except where the kernel picks a scalar path by the pointer (clip_round.x,
               augment_batch.lr/hr/mask, ensemble_expand.lr, ensemble_reduce.sr, tile_blend.sr, frame_windows_gather.patches,
               frame_windows_reduce.sr), which go in as they are; refused for a written operand
  6 sizes      operands against each other and against the engine (engine_sizes: asked once per handle; the fake rule only for a handle already
               known, a trace may carry a placeholder) and the scalars (which, border, pad, ksize, impl, lo <= hi, ...), else ValueError
  7 empty      never reaches the library: empty outputs (clip_round, esa_shift_*, an empty recipe of augment_batch / ensemble_expand / crop_batch),
               a no-op (nadam_step, nadam_step_guarded), ValueError everywhere else (network ops, losses, the other batch reductions)

  limits       out_size of wdsr_forward is the caller's (the C ABI has no query for it); all operands on the CURRENT device (_lib.current_stream()
               takes none)
"""
from ctypes import c_void_p
from typing import Optional

import torch
from torch import Tensor

from . import _lib

# ---------------------------------------------------------------------------------------------------------------------------------
# the argument contract (the module docstring's table; INTEGRATION.md, 'Custom ops: what an op accepts').  Every op has ONE validator
# that its real and its fake implementation share; it runs before any compute entry point of the library.
# ---------------------------------------------------------------------------------------------------------------------------------
IMPLS = {}                    # op name -> the undecorated function behind torch.ops.probav.<name> (tests/ops_contract.py calls these on meta tensors)


def _plain(fn):
    IMPLS[fn.__name__] = fn
    return fn


_F32, _F64, _I32, _I64 = (torch.float32,), (torch.float64,), (torch.int32,), (torch.int64,)
_MASK = (torch.uint8, torch.bool)          # nonzero = set: a bool tensor holds the bytes 0 / 1
_U16 = (torch.uint16, torch.int16)         # int16 is taken as the same bits


def _operands(op, real, *rows):
    """rows of (name, tensor or None, accepted dtypes, rank or None): every tensor operand on ONE device -- a HIP device for the real
    implementation; a fake rule sees only that they agree -- (RuntimeError), each of an accepted dtype and rank (ValueError)."""
    dev = first = None
    for name, t, _, _ in rows:
        if t is None:
            continue
        if real:
            _lib.require_device(t, "%s: %s" % (op, name))
        if dev is None:
            dev, first = t.device, name
        elif t.device != dev:
            raise RuntimeError("%s: %s lives on %s but %s on %s: every tensor operand of an op lives on one HIP device (no CPU fallback)"
                               % (op, name, t.device, first, dev))
    for name, t, dtypes, rank in rows:
        if t is None:
            continue
        if t.dtype not in dtypes:
            raise ValueError("%s: %s must be %s, got %s (operands are never cast)" % (op, name, " or ".join(str(d) for d in dtypes), t.dtype))
        if rank is not None and t.dim() != rank:
            raise ValueError("%s: %s must have %d dimensions, got shape %s" % (op, name, rank, tuple(t.shape)))


def _aligned(t):
    """The view starts on a 16-byte boundary of its allocation (torch's allocators hand out blocks aligned to 512 bytes and more)."""
    return (t.storage_offset() * t.element_size()) % 16 == 0


def _dense(t, any_offset=False):
    """An operand the op only READS, as the kernels want it: dense, row-major, 16-byte aligned (include/probav_hip.h: 'All buffers contiguous,
    16-byte aligned') -- the tensor itself if it is that already, else a copy.  any_offset: the kernel behind this operand picks a scalar path
    by the pointer's alignment (the table names them), so an offset view goes in as it is."""
    if t is None:
        return None
    if not t.is_contiguous():
        return t.contiguous()
    return t if any_offset or _aligned(t) else t.clone()


def _mutated(op, *rows):
    """rows of (name, tensor or None): operands the op WRITES in place cannot be copied -- contiguous and 16-byte aligned, or a ValueError."""
    for name, t in rows:
        if t is None:
            continue
        if not t.is_contiguous():
            raise ValueError("%s: %s is written in place and must be contiguous, got shape %s with strides %s" % (op, name, tuple(t.shape), tuple(t.stride())))
        if not _aligned(t):
            raise ValueError("%s: %s is written in place and must start on a 16-byte boundary, got a view at storage offset %d (%d bytes)"
                             % (op, name, t.storage_offset(), t.storage_offset() * t.element_size()))


def _want(op, ok, text, *args):
    if not ok:
        raise ValueError("%s: %s" % (op, text % args if args else text))


_ENGINE_SIZES = {}            # engine handle -> (param_count, weff_count, cout_total, input shape [1:], weight-cache floats): fixed for the engine's life


def engine_sizes(engine):
    """What the validators hold the operands of an engine op to, asked of the library once per handle (no ctypes round trip per step)."""
    s = _ENGINE_SIZES.get(engine)
    if s is None:
        L, h = _lib.lib(), c_void_p(engine)
        s = (int(L.probav_param_count(h)), int(L.probav_weff_count(h)), int(L.probav_cout_total(h)), tuple(_input_shape(engine, 1)[1:]),
             (int(L.probav_weight_cache_bytes(h)) + 3) // 4)
        _ENGINE_SIZES[engine] = s
    return s


def forget_engine(engine):
    """Drop the cached sizes of a handle: call it when the engine is destroyed (the address may be handed to the next engine) or re-routed."""
    _ENGINE_SIZES.pop(int(engine), None)


def _engine_known(engine, real):
    """The engine's sizes: asked for by a real implementation, only looked up by a fake rule (a trace may carry a placeholder handle, and a fake
    rule must not hand one to the library: it then checks the operands against each other only)."""
    return engine_sizes(engine) if real else _ENGINE_SIZES.get(engine)


# ---------------------------------------------------------------------------------------------------------------------------------
# the network
# ---------------------------------------------------------------------------------------------------------------------------------
_WS_POOLS = {}


def _ws_pool(device, kind="ws"):
    """A private, never-split allocator pool for the engine workspaces (torch.cuda.MemPool): a multi-GB block that returns to the general
    pool gets carved up by the next megabyte-sized request, and the following step then pays a hipMalloc of the full size (~80 ms,
    device-synchronous).  In its own pool a freed workspace block can only be taken by the next workspace.  The reverse pass's scratch
    blocks (kind "scratch") have a pool of their own: a freed 2 GB scratch block must not be handed to the next 2 GB workspace request
    while the following scratch request then finds nothing."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), kind)
    pool = _WS_POOLS.get(key)
    if pool is None:
        try:
            pool = torch.cuda.MemPool(no_split=True)
        except TypeError:                                  # (a torch without the keyword: blocks of this pool may then be split)
            pool = torch.cuda.MemPool()
        _WS_POOLS[key] = pool
    return pool


def release_workspaces(device=None):
    """Return the workspace blocks to the driver.  Every distinct (batch, training, frames) shape pins its own multi-GB block in the
    private pool for as long as the pool lives (a trainer alternating training batches, a partial last batch, validation batches and
    inference micro-batches holds one block each); call this between such phases of a long-lived process.  Blocks still referenced
    (an un-run backward) are freed when their tensors die."""
    dev = None if device is None else (torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device())
    for k in [k for k in _WS_POOLS if dev is None or k[0] == dev]:
        _WS_POOLS.pop(k, None)
    torch.cuda.empty_cache()


def _ws_floats(engine, batch, training):
    """Floats of the workspace wdsr_forward returns: in training mode the SAVED STATE of the pass only (probav_workspace_split) -- the reverse
    pass brings its own scratch."""
    n = _split_floats(engine, batch)[0] if training else (_lib.lib().probav_workspace_bytes(c_void_p(engine), int(batch), 0) + 3) // 4
    if n == 0:
        raise RuntimeError("probav_workspace_bytes returned 0")
    return n


def _split_floats(engine, batch):
    """(saved, scratch) floats of probav_workspace_split: one call answers for the workspace a reverse pass reads and the scratch it brings."""
    import ctypes
    saved, scratch = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.check(_lib.lib().probav_workspace_split(c_void_p(engine), int(batch), ctypes.byref(saved), ctypes.byref(scratch)), "probav_workspace_split")
    return (saved.value + 3) // 4, (scratch.value + 3) // 4


def _wdsr_forward_args(real, flat, x, engine, out_size, training, wcache):
    """-> B after the checks the real and the fake implementation share."""
    op = "wdsr_forward"
    _operands(op, real, ("flat", flat, _F32, None), ("x", x, _F32, 5), ("wcache", wcache, _F32, None))
    B = int(x.shape[0])
    _want(op, B >= 1, "x holds an empty batch, got shape %s (the network ops refuse one)", tuple(x.shape))
    _want(op, out_size >= 1, "out_size = %d, the side of the prediction, must be positive", out_size)
    sizes = _engine_known(engine, real)
    if sizes is not None:
        _want(op, flat.numel() == sizes[0], "flat holds %d values, the engine has %d parameters", flat.numel(), sizes[0])
        _want(op, tuple(x.shape[1:]) == sizes[3], "x must be [B, %d, %d, %d, %d] for this engine, got %s", *(sizes[3] + (tuple(x.shape),)))
        _want(op, wcache is None or wcache.numel() >= sizes[4], "wcache holds %d floats, the engine's weight cache needs %d",
              0 if wcache is None else wcache.numel(), sizes[4])
    return B


@torch.library.custom_op("probav::wdsr_forward", mutates_args=(), device_types="cuda")
@_plain
def wdsr_forward(flat: Tensor, x: Tensor, engine: int, out_size: int, training: bool, wcache: Optional[Tensor] = None) -> tuple[Tensor, Tensor]:
    """-> (y [B, out_size, out_size, 1], ws): ws is the engine workspace of this call -- with training=True it holds the activations the
    reverse pass needs (the op is functional: the saved state is an OUTPUT, like the residuals of any differentiable op).
    wcache (optional): the weight cache probav::optimizer_wn_step filled for exactly these parameters; the weight-norm and packing
    launches are then skipped."""
    B = _wdsr_forward_args(True, flat, x, engine, out_size, training, wcache)
    flat, x, wcache = _dense(flat), _dense(x), _dense(wcache)
    y = torch.empty((B, out_size, out_size, 1), dtype=torch.float32, device=x.device)
    with torch.cuda.use_mem_pool(_ws_pool(x.device), device=x.device):
        ws = torch.empty(_ws_floats(engine, B, training), dtype=torch.float32, device=x.device)
    L = _lib.lib()
    if wcache is None:
        _lib.check(L.probav_forward(c_void_p(engine), _lib.ptr(flat), _lib.ptr(x), _lib.ptr(y), _lib.ptr(ws), ws.numel() * 4, B,
                                    1 if training else 0, _lib.current_stream()), "probav_forward")
    else:
        _lib.check(L.probav_forward_wc(c_void_p(engine), _lib.ptr(flat), _lib.ptr(x), _lib.ptr(y), _lib.ptr(ws), ws.numel() * 4, B,
                                       1 if training else 0, _lib.ptr(wcache), wcache.numel() * 4, _lib.current_stream()), "probav_forward_wc")
    return y, ws


@wdsr_forward.register_fake
def _(flat, x, engine, out_size, training, wcache=None):
    B = _wdsr_forward_args(False, flat, x, engine, out_size, training, wcache)
    return (x.new_empty((B, out_size, out_size, 1), dtype=torch.float32), x.new_empty((_ws_floats(engine, B, training),), dtype=torch.float32))


def _wdsr_backward_args(op, real, flat, dy, ws, engine, wcache):
    """-> (B, scratch floats or None) after the checks the real and the fake implementation of both reverse ops share."""
    _operands(op, real, ("flat", flat, _F32, None), ("dy", dy, _F32, 4), ("ws", ws, _F32, 1), ("wcache", wcache, _F32, None))
    B = int(dy.shape[0])
    _want(op, B >= 1, "dy holds an empty batch, got shape %s (the network ops refuse one)", tuple(dy.shape))
    _want(op, dy.shape[1] == dy.shape[2] and dy.shape[3] == 1 and dy.shape[1] >= 1, "dy must be [B, S, S, 1], got %s", tuple(dy.shape))
    sizes, scratch = _engine_known(engine, real), None
    if sizes is not None:
        _want(op, flat.numel() == sizes[0], "flat holds %d values, the engine has %d parameters", flat.numel(), sizes[0])
        _want(op, wcache is None or wcache.numel() >= sizes[4], "wcache holds %d floats, the engine's weight cache needs %d",
              0 if wcache is None else wcache.numel(), sizes[4])
    if sizes is not None:                      # (a host query of a handle known to be live: the fake rule of a known engine asks it too)
        saved, scratch = _split_floats(engine, B)
        _want(op, ws.numel() == saved, "ws holds %d floats, the saved state of a training pass of batch %d holds %d (pass the workspace "
              "wdsr_forward(training=True) returned for this batch)", ws.numel(), B, saved)
    return B, scratch


@torch.library.custom_op("probav::wdsr_backward", mutates_args=(), device_types="cuda")
@_plain
def wdsr_backward(flat: Tensor, dy: Tensor, ws: Tensor, engine: int, wcache: Optional[Tensor] = None) -> Tensor:
    """d loss / d flat from d loss / d y; `ws` = the saved state the matching forward returned, only READ here (probav_backward_split): the
    reverse pass's gradient buffers and partial-sum slabs live in a scratch block of this call's own, from the same private pool as the
    workspaces.  The op is functional -- a second backward over the same graph (retain_graph, a gradient check) reads the same
    activations, and AOT-autograd traces the formula of wdsr_forward without any storage aliasing.  wcache = the weight cache that
    forward ran from, if any."""
    B, nscratch = _wdsr_backward_args("wdsr_backward", True, flat, dy, ws, engine, wcache)
    flat, dy, ws, wcache = _dense(flat), _dense(dy), _dense(ws), _dense(wcache)
    grads = torch.empty(flat.shape, dtype=torch.float32, device=flat.device)
    with torch.cuda.use_mem_pool(_ws_pool(dy.device, "scratch"), device=dy.device):
        scratch = torch.empty(nscratch, dtype=torch.float32, device=dy.device)
    _lib.check(_lib.lib().probav_backward_split(c_void_p(engine), _lib.ptr(flat), _lib.ptr(dy), _lib.ptr(grads), _lib.ptr(ws), ws.numel() * 4,
                                                _lib.ptr(scratch), scratch.numel() * 4, B, _lib.ptr(wcache),
                                                0 if wcache is None else wcache.numel() * 4, _lib.current_stream()), "probav_backward_split")
    return grads


@wdsr_backward.register_fake
def _(flat, dy, ws, engine, wcache=None):
    _wdsr_backward_args("wdsr_backward", False, flat, dy, ws, engine, wcache)
    return torch.empty_like(flat, memory_format=torch.contiguous_format)


def _input_shape(engine, batch):
    """Shape of the network's input (and of d loss / d x) for `batch` samples: [B, P + maxShift, P + maxShift, T, C], read from the engine's
    layer table (mainConv1's input channels), its plan (the normalised input's size) and the frame count that makes them agree."""
    import ctypes
    L = _lib.lib()
    shp = (ctypes.c_int32 * 5)()
    _lib.check(L.probav_layer_info(c_void_p(engine), 0, None, None, None, None, ctypes.byref(shp)), "probav_layer_info")
    off, cnt = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(L.probav_workspace_view(c_void_p(engine), int(batch), 1, 4, 0, ctypes.byref(off), ctypes.byref(cnt)), "probav_workspace_view")
    r1o, r1c = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(L.probav_workspace_view(c_void_p(engine), int(batch), 1, 3, 0, ctypes.byref(r1o), ctypes.byref(r1c)), "probav_workspace_view")
    C = int(shp[3])
    h1 = int(round((r1c.value / (9 * int(batch))) ** 0.5))             # relu(residConv1): [B, Hin - 2, Hin - 2, 9]
    hin = h1 + 2
    T = cnt.value // (int(batch) * hin * hin * C)
    if h1 * h1 * 9 * int(batch) != r1c.value or T * int(batch) * hin * hin * C != cnt.value:
        raise RuntimeError("probav_workspace_view: the plan's input and residual extents do not factor")
    return (int(batch), hin, hin, int(T), C)


@torch.library.custom_op("probav::wdsr_backward_input", mutates_args=(), device_types="cuda")
@_plain
def wdsr_backward_input(flat: Tensor, dy: Tensor, ws: Tensor, engine: int, wcache: Optional[Tensor] = None) -> tuple[Tensor, Tensor]:
    """-> (d loss / d flat, d loss / d x): wdsr_backward with the input gradient as a second output (probav_backward_input).  The first
    output has the bits wdsr_backward gives; the second costs one more launch at the end of the pass.  Functional like wdsr_backward: `ws`
    is only read, the scratch is this call's own block from the same private pool."""
    B, nscratch = _wdsr_backward_args("wdsr_backward_input", True, flat, dy, ws, engine, wcache)
    flat, dy, ws, wcache = _dense(flat), _dense(dy), _dense(ws), _dense(wcache)
    grads = torch.empty(flat.shape, dtype=torch.float32, device=flat.device)
    dx = torch.empty((B,) + engine_sizes(engine)[3], dtype=torch.float32, device=dy.device)
    with torch.cuda.use_mem_pool(_ws_pool(dy.device, "scratch"), device=dy.device):
        scratch = torch.empty(nscratch, dtype=torch.float32, device=dy.device)
    _lib.check(_lib.lib().probav_backward_input(c_void_p(engine), _lib.ptr(flat), _lib.ptr(dy), _lib.ptr(grads), _lib.ptr(ws), ws.numel() * 4,
                                                _lib.ptr(scratch), scratch.numel() * 4, B, _lib.ptr(wcache),
                                                0 if wcache is None else wcache.numel() * 4, _lib.ptr(dx), _lib.current_stream()), "probav_backward_input")
    return grads, dx


@wdsr_backward_input.register_fake
def _(flat, dy, ws, engine, wcache=None):
    B, _ = _wdsr_backward_args("wdsr_backward_input", False, flat, dy, ws, engine, wcache)
    return torch.empty_like(flat, memory_format=torch.contiguous_format), dy.new_empty(_input_shape(engine, B), dtype=torch.float32)


def _wdsr_setup(ctx, inputs, output):
    flat, x, engine, out_size, training, wcache = inputs
    ctx.wcache = wcache
    # the workspace is an OUTPUT of this node: it must go through save_for_backward (a plain attribute would close the reference cycle
    # node -> ctx -> ws -> grad_fn -> node and every step's 3 GB would stay alive until the cycle collector runs, if ever)
    ctx.save_for_backward(flat, output[1])
    ctx.engine, ctx.training = engine, training
    ctx.mark_non_differentiable(output[1])
    ctx.set_materialize_grads(False)           # ... and it never carries a gradient: do not let autograd zero-fill 3 GB for it


def _wdsr_bwd(ctx, dy, dws):
    if dy is None:
        return None, None, None, None, None, None
    if not ctx.training:
        raise RuntimeError("backward through model(x, training=False): call the model with training=True "
                           "to keep the activations the reverse pass needs")
    flat, ws = ctx.saved_tensors
    if ctx.needs_input_grad[1]:                # d loss / d x asked for: the same pass with one more launch and one more output
        g, dx = torch.ops.probav.wdsr_backward_input(flat, dy.contiguous().float(), ws, ctx.engine, ctx.wcache)
        return g, dx, None, None, None, None
    g = torch.ops.probav.wdsr_backward(flat, dy.contiguous().float(), ws, ctx.engine, ctx.wcache)
    return g, None, None, None, None, None


wdsr_forward.register_autograd(_wdsr_bwd, setup_context=_wdsr_setup)


# ---------------------------------------------------------------------------------------------------------------------------------
# shift-compensated losses / metric (csrc/kernels_loss.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
@torch.library.custom_op("probav::shift_metrics", mutates_args=(), device_types="cuda")
@_plain
def shift_metrics(hr: Tensor, mask: Tensor, pred: Tensor, border: int, bit_depth: int) -> tuple[Tensor, Tensor, Tensor]:
    B, S = _crop_loss_args("shift_metrics", pred, hr, mask, border, 1, real=True)
    pred, hr, mask = _dense(pred), _dense(hr), _dense(mask)
    dev = pred.device
    f = torch.empty((3, B), dtype=torch.float32, device=dev)          # l1 | l2 | cpsnr
    arg = torch.empty((2, B), dtype=torch.int32, device=dev)
    means = torch.empty(2, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().probav_shift_loss_forward(
        _lib.ptr(hr), _lib.ptr(mask), _lib.ptr(pred), B, S, border, bit_depth, _lib.ptr(f[0]), _lib.ptr(f[1]),
        _lib.ptr(f[2]), _lib.ptr(arg[0]), _lib.ptr(arg[1]), _lib.ptr(means[0:1]), _lib.ptr(means[1:2]),
        _lib.current_stream()), "probav_shift_loss_forward")
    return f, arg, means


@shift_metrics.register_fake
def _(hr, mask, pred, border, bit_depth):
    B, _ = _crop_loss_args("shift_metrics", pred, hr, mask, border, 1)
    return (pred.new_empty((3, B), dtype=torch.float32), pred.new_empty((2, B), dtype=torch.int32), pred.new_empty((2,), dtype=torch.float32))


@torch.library.custom_op("probav::shift_loss_backward", mutates_args=(), device_types="cuda")
@_plain
def shift_loss_backward(hr: Tensor, mask: Tensor, pred: Tensor, arg: Tensor, upstream: Tensor, border: int, which: int) -> Tensor:
    B, S = _crop_loss_backward_args("shift_loss_backward", pred, hr, mask, arg, None, upstream, border, 1, real=True)
    _want("shift_loss_backward", which in (1, 2), "which = %r; 1 = L1, 2 = L2", which)
    pred, hr, mask, arg, upstream = _dense(pred), _dense(hr), _dense(mask), _dense(arg), _dense(upstream)
    dpred = torch.empty_like(pred)
    _lib.check(_lib.lib().probav_shift_loss_backward(
        _lib.ptr(hr), _lib.ptr(mask), _lib.ptr(pred), _lib.ptr(arg), B, S, border,
        which, _lib.ptr(upstream), _lib.ptr(dpred), _lib.current_stream()), "probav_shift_loss_backward")
    return dpred


@shift_loss_backward.register_fake
def _(hr, mask, pred, arg, upstream, border, which):
    _crop_loss_backward_args("shift_loss_backward", pred, hr, mask, arg, None, upstream, border, 1)
    _want("shift_loss_backward", which in (1, 2), "which = %r; 1 = L1, 2 = L2", which)
    return torch.empty_like(pred, memory_format=torch.contiguous_format)


@torch.library.custom_op("probav::shift_loss", mutates_args=(), device_types="cuda")
@_plain
def shift_loss(pred: Tensor, hr: Tensor, mask: Tensor, border: int, bit_depth: int, which: int) -> tuple[Tensor, Tensor, Tensor]:
    """which = 1: L1 (models/loss.py:73-84), 2: L2 (:55-71) -> (batch-mean loss [scalar], arg-min shift per sample [B], per-sample minima [B])."""
    # the launch writes through seven separate pointers: the three results asked for go straight into tensors of their own (no copies: three
    # launches less per step), the other four into one scratch allocation
    B, S = _crop_loss_args("shift_loss", pred, hr, mask, border, 1, real=True)
    _want("shift_loss", which in (1, 2), "which = %r; 1 = L1, 2 = L2", which)
    pred, hr, mask = _dense(pred), _dense(hr), _dense(mask)
    dev = pred.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    amin = torch.empty((B,), dtype=torch.int32, device=dev)
    per = torch.empty((B,), dtype=torch.float32, device=dev)
    scr = torch.empty((2 * B + 1,), dtype=torch.float32, device=dev)        # the other per-sample loss, cPSNR, the other mean
    sarg = torch.empty((B,), dtype=torch.int32, device=dev)
    l1 = which == 1
    _lib.check(_lib.lib().probav_shift_loss_forward(
        _lib.ptr(hr), _lib.ptr(mask), _lib.ptr(pred), B, S, border, bit_depth,
        _lib.ptr(per if l1 else scr[0:B]), _lib.ptr(scr[0:B] if l1 else per), _lib.ptr(scr[B:2 * B]),
        _lib.ptr(amin if l1 else sarg), _lib.ptr(sarg if l1 else amin),
        _lib.ptr(loss if l1 else scr[2 * B:]), _lib.ptr(scr[2 * B:] if l1 else loss),
        _lib.current_stream()), "probav_shift_loss_forward")
    return loss, amin, per


@shift_loss.register_fake
def _(pred, hr, mask, border, bit_depth, which):
    B, _ = _crop_loss_args("shift_loss", pred, hr, mask, border, 1)
    _want("shift_loss", which in (1, 2), "which = %r; 1 = L1, 2 = L2", which)
    return (pred.new_empty((), dtype=torch.float32), pred.new_empty((B,), dtype=torch.int32), pred.new_empty((B,), dtype=torch.float32))


def _shift_setup(ctx, inputs, output):
    pred, hr, mask, border, bit_depth, which = inputs
    ctx.save_for_backward(pred, hr, mask, output[1])
    ctx.border, ctx.which = border, which
    ctx.set_materialize_grads(False)


def _shift_bwd(ctx, g_loss, g_arg, g_per):
    if g_loss is None:                         # (only the batch-mean loss is differentiable; the per-sample minima are a by-product)
        return None, None, None, None, None, None
    pred, hr, mask, arg = ctx.saved_tensors
    dpred = torch.ops.probav.shift_loss_backward(hr, mask, pred, arg, g_loss.contiguous().float().reshape(1), ctx.border, ctx.which)
    return dpred, None, None, None, None, None


shift_loss.register_autograd(_shift_bwd, setup_context=_shift_setup)


def _crop_loss_args(name, pred, hr, mask, border, min_crop, real=False, more=()):
    """-> (B, S) after the checks the real and the fake implementation of a shift-compensated loss share (mask: nonzero = clear)."""
    _operands(name, real, ("pred", pred, _F32, 4), ("hr", hr, _F32, 4), ("mask", mask, _MASK, 4), *more)
    if pred.shape[3] != 1 or pred.shape[1] != pred.shape[2] or hr.shape != pred.shape or mask.shape != pred.shape:
        raise ValueError("%s: pred, hr, mask must all be [B, S, S, 1]; got %s %s %s" % (name, tuple(pred.shape), tuple(hr.shape), tuple(mask.shape)))
    B, S = int(pred.shape[0]), int(pred.shape[1])
    if B < 1:
        raise ValueError("%s: pred, hr, mask hold an empty batch (a batch mean needs a sample), got %s" % (name, tuple(pred.shape)))
    if border < 0 or S - 2 * border < min_crop:
        raise ValueError("%s: bad shape (border = %d must not be negative and the crop = size - 2 * border = %d must be at least %d)"
                         % (name, border, S - 2 * border, min_crop))
    return B, S


def _crop_loss_backward_args(name, pred, hr, mask, arg, n_arg, upstream, border, min_crop, real=False, more=()):
    B, S = _crop_loss_args(name, pred, hr, mask, border, min_crop, real, (("arg", arg, _I32, None), ("upstream", upstream, _F32, None)) + tuple(more))
    if arg.numel() != (B if n_arg is None else n_arg) or upstream.numel() != 1:
        raise ValueError("%s: arg int32 [%d], upstream float32 [1]; got %s, %s" % (name, B if n_arg is None else n_arg, tuple(arg.shape), tuple(upstream.shape)))
    return B, S


@torch.library.custom_op("probav::shift_l1edge_loss", mutates_args=(), device_types="cuda")
@_plain
def shift_l1edge_loss(pred: Tensor, hr: Tensor, mask: Tensor, border: int, pi: float) -> tuple[Tensor, Tensor, Tensor]:
    """cfg loss = sobel_l1_mix (models/loss.py:86-97): pi * L1 + (1 - pi) * Sobel-edge L1 of the bias-corrected residual, minimum over the shifts
    -> (batch-mean loss [scalar], arg-min shift per sample [B], per-sample minima [B]).  Two launches: all shifts of every sample, the batch mean."""
    B, S = _crop_loss_args("shift_l1edge_loss", pred, hr, mask, border, 3, real=True)
    pred, hr, mask = _dense(pred), _dense(hr), _dense(mask)
    per = torch.empty((B,), dtype=torch.float32, device=pred.device)
    arg = torch.empty((B,), dtype=torch.int32, device=pred.device)
    mean = torch.empty((2,), dtype=torch.float32, device=pred.device)       # the C entry point's mean[2]: the loss and a scratch word
    _lib.check(_lib.lib().probav_shift_l1edge_forward(_lib.ptr(hr), _lib.ptr(mask), _lib.ptr(pred), B, S, border, pi, _lib.ptr(per), _lib.ptr(arg),
                                                      _lib.ptr(mean), _lib.current_stream()), "probav_shift_l1edge_forward")
    return mean[0], arg, per                   # (a 0-dim view of this call's own allocation: no copy launch)


@shift_l1edge_loss.register_fake
def _(pred, hr, mask, border, pi):
    B, _ = _crop_loss_args("shift_l1edge_loss", pred, hr, mask, border, 3)
    return (pred.new_empty((), dtype=torch.float32), pred.new_empty((B,), dtype=torch.int32), pred.new_empty((B,), dtype=torch.float32))


@torch.library.custom_op("probav::shift_l1edge_loss_backward", mutates_args=(), device_types="cuda")
@_plain
def shift_l1edge_loss_backward(hr: Tensor, mask: Tensor, pred: Tensor, arg: Tensor, upstream: Tensor, border: int, pi: float) -> Tensor:
    B, S = _crop_loss_backward_args("shift_l1edge_loss_backward", pred, hr, mask, arg, None, upstream, border, 3, real=True)
    pred, hr, mask, arg, upstream = _dense(pred), _dense(hr), _dense(mask), _dense(arg), _dense(upstream)
    dpred = torch.empty_like(pred)
    _lib.check(_lib.lib().probav_shift_l1edge_backward(_lib.ptr(hr), _lib.ptr(mask), _lib.ptr(pred), _lib.ptr(arg), B, S, border, pi, _lib.ptr(upstream),
                                                       _lib.ptr(dpred), _lib.current_stream()), "probav_shift_l1edge_backward")
    return dpred


@shift_l1edge_loss_backward.register_fake
def _(hr, mask, pred, arg, upstream, border, pi):
    _crop_loss_backward_args("shift_l1edge_loss_backward", pred, hr, mask, arg, None, upstream, border, 3)
    return torch.empty_like(pred, memory_format=torch.contiguous_format)


def _l1edge_setup(ctx, inputs, output):
    pred, hr, mask, border, pi = inputs
    ctx.save_for_backward(pred, hr, mask, output[1])
    ctx.border, ctx.pi = border, pi
    ctx.set_materialize_grads(False)


def _l1edge_bwd(ctx, g_loss, g_arg, g_per):
    if g_loss is None:                         # (only the batch-mean loss is differentiable)
        return None, None, None, None, None
    pred, hr, mask, arg = ctx.saved_tensors
    dpred = torch.ops.probav.shift_l1edge_loss_backward(hr, mask, pred, arg, g_loss.contiguous().float().reshape(1), ctx.border, ctx.pi)
    return dpred, None, None, None, None


shift_l1edge_loss.register_autograd(_l1edge_bwd, setup_context=_l1edge_setup)

REVSSIM_SCALES, REVSSIM_SUMS = 5, 7            # csrc/kernels_loss.hip: the weighted sums one (shift, sample, scale) leaves for the reverse pass


def _revssim_moments_shape(B, border):
    ns = 2 * border + 1
    return (ns * ns, B, REVSSIM_SCALES, REVSSIM_SUMS)


@torch.library.custom_op("probav::revssim_loss", mutates_args=(), device_types="cuda")
@_plain
def revssim_loss(pred: Tensor, hr: Tensor, mask: Tensor, border: int, bit_depth: int, eta: float) -> tuple[Tensor, Tensor, Tensor]:
    """cfg loss = l1msssim (models/loss.py:99-124, 189-212): the batch-level multi-scale SSIM / weighted-L1 mixture, minimum over the shifts
    -> (loss [scalar], the batch's arg-min shift [1], moments float64 [shifts, B, 5, 7]).  `moments` is the saved state of the pass: an OUTPUT
    here (like wdsr_forward's workspace), an input of revssim_loss_backward; every element is written."""
    B, S = _crop_loss_args("revssim_loss", pred, hr, mask, border, 2, real=True)
    pred, hr, mask = _dense(pred), _dense(hr), _dense(mask)
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    arg = torch.empty((1,), dtype=torch.int32, device=pred.device)
    moments = torch.empty(_revssim_moments_shape(B, border), dtype=torch.float64, device=pred.device)
    nbytes = _lib.lib().probav_revssim_scratch_bytes(B, border)
    if moments.numel() * 8 != nbytes:
        raise RuntimeError("revssim_loss: moments of %d bytes, probav_revssim_scratch_bytes(%d, %d) = %d" % (moments.numel() * 8, B, border, nbytes))
    _lib.check(_lib.lib().probav_revssim_forward(_lib.ptr(hr), _lib.ptr(mask), _lib.ptr(pred), B, S, border, bit_depth, eta, _lib.ptr(moments),
                                                 nbytes, _lib.ptr(loss), _lib.ptr(arg), _lib.current_stream()), "probav_revssim_forward")
    return loss, arg, moments


@revssim_loss.register_fake
def _(pred, hr, mask, border, bit_depth, eta):
    B, _ = _crop_loss_args("revssim_loss", pred, hr, mask, border, 2)
    return (pred.new_empty((), dtype=torch.float32), pred.new_empty((1,), dtype=torch.int32),
            pred.new_empty(_revssim_moments_shape(B, border), dtype=torch.float64))


def _revssim_backward_args(hr, mask, pred, arg, moments, upstream, border, real=False):
    B, S = _crop_loss_backward_args("revssim_loss_backward", pred, hr, mask, arg, 1, upstream, border, 2, real, (("moments", moments, _F64, None),))
    if tuple(moments.shape) != _revssim_moments_shape(B, border):
        raise ValueError("revssim_loss_backward: moments must be the float64 %s that revssim_loss returned; got %s"
                         % (_revssim_moments_shape(B, border), tuple(moments.shape)))
    return B, S


@torch.library.custom_op("probav::revssim_loss_backward", mutates_args=(), device_types="cuda")
@_plain
def revssim_loss_backward(hr: Tensor, mask: Tensor, pred: Tensor, arg: Tensor, moments: Tensor, upstream: Tensor, border: int, bit_depth: int,
                          eta: float) -> Tensor:
    B, S = _revssim_backward_args(hr, mask, pred, arg, moments, upstream, border, real=True)
    pred, hr, mask, arg, moments, upstream = _dense(pred), _dense(hr), _dense(mask), _dense(arg), _dense(moments), _dense(upstream)
    dpred = torch.empty_like(pred)
    _lib.check(_lib.lib().probav_revssim_backward(_lib.ptr(hr), _lib.ptr(mask), _lib.ptr(pred), _lib.ptr(arg), _lib.ptr(moments), B, S, border, bit_depth,
                                                  eta, _lib.ptr(upstream), _lib.ptr(dpred), _lib.current_stream()), "probav_revssim_backward")
    return dpred


@revssim_loss_backward.register_fake
def _(hr, mask, pred, arg, moments, upstream, border, bit_depth, eta):
    _revssim_backward_args(hr, mask, pred, arg, moments, upstream, border)
    return torch.empty_like(pred, memory_format=torch.contiguous_format)


def _revssim_setup(ctx, inputs, output):
    pred, hr, mask, border, bit_depth, eta = inputs
    ctx.save_for_backward(pred, hr, mask, output[1], output[2])      # (moments is an output of this node: through save_for_backward, see _wdsr_setup)
    ctx.border, ctx.bit_depth, ctx.eta = border, bit_depth, eta
    ctx.mark_non_differentiable(output[1], output[2])
    ctx.set_materialize_grads(False)


def _revssim_bwd(ctx, g_loss, g_arg, g_moments):
    if g_loss is None:
        return None, None, None, None, None, None
    pred, hr, mask, arg, moments = ctx.saved_tensors
    dpred = torch.ops.probav.revssim_loss_backward(hr, mask, pred, arg, moments, g_loss.contiguous().float().reshape(1), ctx.border, ctx.bit_depth, ctx.eta)
    return dpred, None, None, None, None, None


revssim_loss.register_autograd(_revssim_bwd, setup_context=_revssim_setup)


# ---------------------------------------------------------------------------------------------------------------------------------
# optimizer update, inference epilogue
# ---------------------------------------------------------------------------------------------------------------------------------
GUARD_CTL_WORDS = 4           # struct probav_guard_ctl as an int32 tensor: [scale (f32 bits), skip, skipped_total, norm (f32 bits)]


def guard_scratch_doubles(n):
    """float64 elements of the scratch probav::grad_guard needs for a gradient of n floats (probav_grad_guard_scratch_bytes)."""
    return (_lib.lib().probav_grad_guard_scratch_bytes(int(n)) + 7) // 8


def _optim_args(op, real, theta, grad, m, v, wcache=None, ema=None, ctl=None, engine=None):
    """-> n after the checks the real and the fake implementation of an optimizer op share: theta, m, v (wcache, ema, ctl) are written in
    place -- contiguous, aligned, never copied; grad is only read."""
    _operands(op, real, ("theta", theta, _F32, None), ("grad", grad, _F32, None), ("m", m, _F32, None), ("v", v, _F32, None),
              ("wcache", wcache, _F32, None), ("ema", ema, _F32, None), ("ctl", ctl, _I32, None))
    n = theta.numel()
    for name, t in (("grad", grad), ("m", m), ("v", v), ("ema", ema)):
        _want(op, t is None or t.numel() == n, "%s holds %d values, theta %d", name, 0 if t is None else t.numel(), n)
    _want(op, ctl is None or ctl.numel() == GUARD_CTL_WORDS, "ctl must hold the %d int32 words of struct probav_guard_ctl, got shape %s",
          GUARD_CTL_WORDS, None if ctl is None else tuple(ctl.shape))
    _mutated(op, ("theta", theta), ("m", m), ("v", v), ("wcache", wcache), ("ema", ema), ("ctl", ctl))
    if engine is not None:
        sizes = _engine_known(engine, real)
        if sizes is not None:
            _want(op, n == sizes[0], "theta holds %d values, the engine has %d parameters", n, sizes[0])
            _want(op, wcache.numel() >= sizes[4], "wcache holds %d floats, the engine's weight cache needs %d", wcache.numel(), sizes[4])
    return n


@torch.library.custom_op("probav::nadam_step", mutates_args=("theta", "m", "v"), device_types="cuda")
@_plain
def nadam_step(theta: Tensor, grad: Tensor, m: Tensor, v: Tensor, lr: float, beta_1: float, beta_2: float, eps: float,
               c_g: float, c_m: float, c_v: float) -> None:
    n = _optim_args("nadam_step", True, theta, grad, m, v)
    if n == 0:                                 # nothing to update: an empty parameter never reaches the library
        return
    _lib.check(_lib.lib().probav_nadam_step(_lib.ptr(theta), _lib.ptr(_dense(grad)), _lib.ptr(m), _lib.ptr(v), n, lr, beta_1, beta_2, eps,
                                            c_g, c_m, c_v, _lib.current_stream()), "probav_nadam_step")


@nadam_step.register_fake
def _(theta, grad, m, v, lr, beta_1, beta_2, eps, c_g, c_m, c_v):
    _optim_args("nadam_step", False, theta, grad, m, v)
    return None


@torch.library.custom_op("probav::optimizer_wn_step", mutates_args=("theta", "m", "v", "wcache"), device_types="cuda")
@_plain
def optimizer_wn_step(theta: Tensor, grad: Tensor, m: Tensor, v: Tensor, wcache: Tensor, engine: int, lr: float, beta_1: float, beta_2: float,
                      eps: float, c_g: float, c_m: float, c_v: float) -> None:
    """nadam_step on the engine's flat parameter buffer, fused with the weight normalisation (and operand packing) of the UPDATED
    parameters into `wcache` (probav_weight_cache_bytes): the next wdsr_forward(..., wcache) starts at its first convolution."""
    _optim_args("optimizer_wn_step", True, theta, grad, m, v, wcache, engine=engine)
    _lib.check(_lib.lib().probav_optimizer_step_fused(c_void_p(engine), _lib.ptr(theta), _lib.ptr(_dense(grad)), _lib.ptr(m), _lib.ptr(v), lr, beta_1, beta_2,
                                                      eps, c_g, c_m, c_v, _lib.ptr(wcache), wcache.numel() * 4, _lib.current_stream()),
               "probav_optimizer_step_fused")


@optimizer_wn_step.register_fake
def _(theta, grad, m, v, wcache, engine, lr, beta_1, beta_2, eps, c_g, c_m, c_v):
    _optim_args("optimizer_wn_step", False, theta, grad, m, v, wcache, engine=engine)
    return None


def _grad_guard_args(real, grad, ctl, scratch):
    op = "grad_guard"
    _operands(op, real, ("grad", grad, _F32, None), ("ctl", ctl, _I32, None), ("scratch", scratch, _F64, None))
    _want(op, grad.numel() >= 1, "grad is empty: the norm of no gradient is not formed")
    _want(op, ctl.numel() == GUARD_CTL_WORDS, "ctl must hold the %d int32 words of struct probav_guard_ctl, got shape %s", GUARD_CTL_WORDS, tuple(ctl.shape))
    need = guard_scratch_doubles(grad.numel())
    _want(op, scratch.numel() >= need, "scratch holds %d float64 values, guard_scratch_doubles(%d) = %d", scratch.numel(), grad.numel(), need)
    _mutated(op, ("ctl", ctl), ("scratch", scratch))


@torch.library.custom_op("probav::grad_guard", mutates_args=("ctl", "scratch"), device_types="cuda")
@_plain
def grad_guard(grad: Tensor, ctl: Tensor, scratch: Tensor, clipnorm: float, skip_nonfinite: bool) -> None:
    """The step's control block from the flat gradient (Keras global_clipnorm = tf.clip_by_global_norm, plus the non-finite guard): fp64 sum of
    squares in a fixed order -> ctl = {scale = clipnorm / max(norm, clipnorm) (1 when clipnorm <= 0), skip, skipped_total += skip, norm}.  Two
    launches; nothing comes back to the host.  ctl: int32 [4], zeroed once by the caller; scratch: float64 [guard_scratch_doubles(n)]."""
    _grad_guard_args(True, grad, ctl, scratch)
    grad = _dense(grad)
    _lib.check(_lib.lib().probav_grad_guard(_lib.ptr(grad), grad.numel(), clipnorm, 1 if skip_nonfinite else 0, _lib.ptr(scratch), scratch.numel() * 8,
                                            _lib.ptr(ctl), _lib.current_stream()), "probav_grad_guard")


@grad_guard.register_fake
def _(grad, ctl, scratch, clipnorm, skip_nonfinite):
    _grad_guard_args(False, grad, ctl, scratch)
    return None


@torch.library.custom_op("probav::nadam_step_guarded", mutates_args=("theta", "m", "v", "ema"), device_types="cuda")
@_plain
def nadam_step_guarded(theta: Tensor, grad: Tensor, m: Tensor, v: Tensor, ema: Optional[Tensor], ctl: Optional[Tensor], lr: float, beta_1: float,
                       beta_2: float, eps: float, c_g: float, c_m: float, c_v: float, ema_momentum: float) -> None:
    """nadam_step on g * ctl.scale, dropped when ctl.skip is set, followed by ema = ema_momentum * ema + (1 - ema_momentum) * theta (Keras use_ema)."""
    n = _optim_args("nadam_step_guarded", True, theta, grad, m, v, None, ema, ctl)
    if n == 0:
        return
    _lib.check(_lib.lib().probav_nadam_step_guarded(_lib.ptr(theta), _lib.ptr(_dense(grad)), _lib.ptr(m), _lib.ptr(v), _lib.ptr(ema), n, lr, beta_1,
                                                    beta_2, eps, c_g, c_m, c_v, ema_momentum, _lib.ptr(ctl), _lib.current_stream()),
               "probav_nadam_step_guarded")


@nadam_step_guarded.register_fake
def _(theta, grad, m, v, ema, ctl, lr, beta_1, beta_2, eps, c_g, c_m, c_v, ema_momentum):
    _optim_args("nadam_step_guarded", False, theta, grad, m, v, None, ema, ctl)
    return None


@torch.library.custom_op("probav::optimizer_wn_step_guarded", mutates_args=("theta", "m", "v", "wcache", "ema"), device_types="cuda")
@_plain
def optimizer_wn_step_guarded(theta: Tensor, grad: Tensor, m: Tensor, v: Tensor, wcache: Tensor, ema: Optional[Tensor], ctl: Optional[Tensor],
                              engine: int, lr: float, beta_1: float, beta_2: float, eps: float, c_g: float, c_m: float, c_v: float,
                              ema_momentum: float) -> None:
    """optimizer_wn_step under the control block and with the EMA buffer: on a skipped step the parameters, both moments and the EMA are left as
    they were and `wcache` is rebuilt from the unchanged parameters (it stays valid)."""
    _optim_args("optimizer_wn_step_guarded", True, theta, grad, m, v, wcache, ema, ctl, engine)
    _lib.check(_lib.lib().probav_optimizer_step_fused_guarded(c_void_p(engine), _lib.ptr(theta), _lib.ptr(_dense(grad)), _lib.ptr(m), _lib.ptr(v), lr, beta_1,
                                                              beta_2, eps, c_g, c_m, c_v, _lib.ptr(wcache), wcache.numel() * 4, _lib.ptr(ema),
                                                              ema_momentum, _lib.ptr(ctl), _lib.current_stream()),
               "probav_optimizer_step_fused_guarded")


@optimizer_wn_step_guarded.register_fake
def _(theta, grad, m, v, wcache, ema, ctl, engine, lr, beta_1, beta_2, eps, c_g, c_m, c_v, ema_momentum):
    _optim_args("optimizer_wn_step_guarded", False, theta, grad, m, v, wcache, ema, ctl, engine)
    return None


def _weight_cache_build_args(real, theta, wcache, engine):
    op = "weight_cache_build"
    _operands(op, real, ("theta", theta, _F32, None), ("wcache", wcache, _F32, None))
    _mutated(op, ("wcache", wcache))
    sizes = _engine_known(engine, real)
    if sizes is not None:
        _want(op, theta.numel() == sizes[0], "theta holds %d values, the engine has %d parameters", theta.numel(), sizes[0])
        _want(op, wcache.numel() >= sizes[4], "wcache holds %d floats, the engine's weight cache needs %d", wcache.numel(), sizes[4])


@torch.library.custom_op("probav::weight_cache_build", mutates_args=("wcache",), device_types="cuda")
@_plain
def weight_cache_build(theta: Tensor, wcache: Tensor, engine: int) -> None:
    """Weight normalisation + operand packing of the CURRENT parameters into `wcache`, for forwards on weights nothing is updating."""
    _weight_cache_build_args(True, theta, wcache, engine)
    _lib.check(_lib.lib().probav_weight_cache_build(c_void_p(engine), _lib.ptr(_dense(theta)), _lib.ptr(wcache), wcache.numel() * 4, _lib.current_stream()),
               "probav_weight_cache_build")


@weight_cache_build.register_fake
def _(theta, wcache, engine):
    _weight_cache_build_args(False, theta, wcache, engine)
    return None


def _clip_round_args(real, x, lo, hi):
    _operands("clip_round", real, ("x", x, _F32, None))
    _want("clip_round", lo <= hi, "lo = %r, hi = %r: lo <= hi, neither a NaN", lo, hi)


@torch.library.custom_op("probav::clip_round", mutates_args=(), device_types="cuda")
@_plain
def clip_round(x: Tensor, lo: float, hi: float) -> Tensor:
    _clip_round_args(True, x, lo, hi)
    x = _dense(x, any_offset=True)             # (csrc/image_math.h picks its scalar path by the pointers)
    out = torch.empty_like(x)
    if x.numel():
        _lib.check(_lib.lib().probav_clip_round(_lib.ptr(x), _lib.ptr(out), x.numel(), lo, hi, _lib.current_stream()), "probav_clip_round")
    return out


@clip_round.register_fake
def _(x, lo, hi):
    _clip_round_args(False, x, lo, hi)
    return torch.empty_like(x, memory_format=torch.contiguous_format)


# ---------------------------------------------------------------------------------------------------------------------------------
# scoring: the ESA shift-compensated clear PSNR of whole images (csrc/kernels_score.hip; the metric is stated in scoring.py).  No
# autograd: a score, not a loss.  sr / hr: [N, S, S] uint16 (int16 is taken as the same bits); mask: [N, S, S] bool or uint8, nonzero = clear.
# ---------------------------------------------------------------------------------------------------------------------------------
def _score_args(op, real, sr, hr, mask, border, min_crop=1):
    """-> (N, S) after the checks the real and the fake implementation of the four scoring ops share."""
    _operands(op, real, ("sr", sr, _U16, 3), ("hr", hr, _U16, 3), ("mask", mask, _MASK, 3))
    if sr.shape[1] != sr.shape[2] or hr.shape != sr.shape or mask.shape != sr.shape:
        raise ValueError("%s: sr, hr, mask must all be [N, S, S]; got %s %s %s" % (op, tuple(sr.shape), tuple(hr.shape), tuple(mask.shape)))
    if not 0 <= border <= 3:
        raise ValueError("%s: border must be in 0..3, got %d" % (op, border))
    N, S = int(sr.shape[0]), int(sr.shape[1])
    if min_crop == 11 and S < 2 * border + 11:
        raise ValueError("%s: the 11-tap window needs 11 rows of the crop: S >= 2 border + 11 = %d, got S = %d" % (op, 2 * border + 11, S))
    _want(op, S - 2 * border >= 1, "sr, hr, mask of side %d leave no crop inside a border of %d", S, border)
    return N, S


def _score_moments(sr, hr, mask, border):
    """(n, s1, s2) of every shift from validated, dense operands: shared by the ops that start from the moments."""
    ns = 2 * border + 1
    mom = torch.empty((sr.shape[0], ns * ns, 3), dtype=torch.int64, device=sr.device)
    if sr.shape[0]:
        _lib.check(_lib.lib().probav_score_moments(_lib.ptr(sr), _lib.ptr(hr), _lib.ptr(mask), sr.shape[0], sr.shape[1], border, _lib.ptr(mom),
                                                   _lib.current_stream()), "probav_score_moments")
    return mom


@torch.library.custom_op("probav::esa_shift_moments", mutates_args=(), device_types="cuda")
@_plain
def esa_shift_moments(sr: Tensor, hr: Tensor, mask: Tensor, border: int) -> Tensor:
    _score_args("esa_shift_moments", True, sr, hr, mask, border)
    return _score_moments(_dense(sr), _dense(hr), _dense(mask), border)


@esa_shift_moments.register_fake
def _(sr, hr, mask, border):
    N, _ = _score_args("esa_shift_moments", False, sr, hr, mask, border)
    ns = 2 * border + 1
    return sr.new_empty((N, ns * ns, 3), dtype=torch.int64)


@torch.library.custom_op("probav::esa_shift_cpsnr", mutates_args=(), device_types="cuda")
@_plain
def esa_shift_cpsnr(sr: Tensor, hr: Tensor, mask: Tensor, border: int) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    N, _ = _score_args("esa_shift_cpsnr", True, sr, hr, mask, border)
    dev = sr.device
    mom = _score_moments(_dense(sr), _dense(hr), _dense(mask), border)
    cpsnr = torch.empty(N, dtype=torch.float64, device=dev)
    shift = torch.empty((N, 2), dtype=torch.int32, device=dev)
    bias = torch.empty(N, dtype=torch.float64, device=dev)
    n_clear = torch.empty(N, dtype=torch.int64, device=dev)
    if N:
        _lib.check(_lib.lib().probav_score_select(_lib.ptr(mom), N, border, _lib.ptr(cpsnr), _lib.ptr(shift), _lib.ptr(bias), _lib.ptr(n_clear),
                                                  _lib.current_stream()), "probav_score_select")
    return cpsnr, shift, bias, n_clear


@esa_shift_cpsnr.register_fake
def _(sr, hr, mask, border):
    N, _ = _score_args("esa_shift_cpsnr", False, sr, hr, mask, border)
    return (sr.new_empty((N,), dtype=torch.float64), sr.new_empty((N, 2), dtype=torch.int32), sr.new_empty((N,), dtype=torch.float64),
            sr.new_empty((N,), dtype=torch.int64))


# the shift-compensated SSIM of the same images (csrc/kernels_ssim.hip; stated in scoring.py).  The 11 Gaussian taps are scoring.gauss11():
# made once on the host in numpy fp64 and handed to the kernel as data, so the numpy statement and the kernel use the same bit patterns.
_GAUSS11 = {}


def _gauss11(device):
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _GAUSS11:
        from .scoring import gauss11
        _GAUSS11[key] = torch.from_numpy(gauss11()).to(device)
    return _GAUSS11[key]


@torch.library.custom_op("probav::esa_shift_ssim_table", mutates_args=(), device_types="cuda")
@_plain
def esa_shift_ssim_table(sr: Tensor, hr: Tensor, mask: Tensor, border: int) -> Tensor:
    _score_args("esa_shift_ssim_table", True, sr, hr, mask, border, 11)
    return _ssim_table(_dense(sr), _dense(hr), _dense(mask), border)


def _ssim_table(sr, hr, mask, border):
    """The windowed SSIM of every shift from validated, dense operands: shared by esa_shift_ssim_table and esa_shift_cssim."""
    N, S, ns = sr.shape[0], sr.shape[1], 2 * border + 1
    table = torch.empty((N, ns * ns), dtype=torch.float64, device=sr.device)
    if N:
        mom = _score_moments(sr, hr, mask, border)
        nbytes = _lib.lib().probav_ssim_scratch_bytes(N, S, border)
        scratch = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=sr.device)
        _lib.check(_lib.lib().probav_ssim_table(_lib.ptr(sr), _lib.ptr(hr), _lib.ptr(mask), _lib.ptr(mom), _lib.ptr(_gauss11(sr.device)), N, S, border,
                                                _lib.ptr(scratch), nbytes, _lib.ptr(table), _lib.current_stream()), "probav_ssim_table")
    return table


@esa_shift_ssim_table.register_fake
def _(sr, hr, mask, border):
    N, _ = _score_args("esa_shift_ssim_table", False, sr, hr, mask, border, 11)
    ns = 2 * border + 1
    return sr.new_empty((N, ns * ns), dtype=torch.float64)


@torch.library.custom_op("probav::esa_shift_cssim", mutates_args=(), device_types="cuda")
@_plain
def esa_shift_cssim(sr: Tensor, hr: Tensor, mask: Tensor, border: int) -> tuple[Tensor, Tensor]:
    N, _ = _score_args("esa_shift_cssim", True, sr, hr, mask, border, 11)
    dev = sr.device
    table = _ssim_table(_dense(sr), _dense(hr), _dense(mask), border)
    cssim = torch.empty(N, dtype=torch.float64, device=dev)
    shift = torch.empty((N, 2), dtype=torch.int32, device=dev)
    if N:
        _lib.check(_lib.lib().probav_ssim_select(_lib.ptr(table), N, border, _lib.ptr(cssim), _lib.ptr(shift), _lib.current_stream()),
                   "probav_ssim_select")
    return cssim, shift


@esa_shift_cssim.register_fake
def _(sr, hr, mask, border):
    N, _ = _score_args("esa_shift_cssim", False, sr, hr, mask, border, 11)
    return sr.new_empty((N,), dtype=torch.float64), sr.new_empty((N, 2), dtype=torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# batch augmentation (csrc/kernels_augment.hip; the recipes are made and validated in augment.py).  No autograd: it moves input bits.
# lr [N, H, H, T, C] fp32, hr [N, S, S, 1] fp32, mask [N, S, S, 1] bool or uint8, recipe [B, 3 + T] int32 rows {i, f, k, perm}.
# ---------------------------------------------------------------------------------------------------------------------------------
def _augment_args(lr, hr, mask, recipe, real=False):
    _operands("augment_batch", real, ("lr", lr, _F32, None), ("hr", hr, _F32, None), ("mask", mask, _MASK, None), ("recipe", recipe, _I32, None))
    if lr.dim() != 5 or hr.dim() != 4 or mask.shape != hr.shape or hr.shape[3] != 1 or hr.shape[0] != lr.shape[0] or recipe.dim() != 2:
        raise ValueError("augment_batch: lr [N, H, H, T, C], hr / mask [N, S, S, 1], recipe [B, 3 + T]; got %s %s %s %s"
                         % (tuple(lr.shape), tuple(hr.shape), tuple(mask.shape), tuple(recipe.shape)))
    if lr.shape[1] != lr.shape[2] or hr.shape[1] != hr.shape[2]:
        raise ValueError("augment_batch: square patches only (a quarter turn needs them); got lr %s, hr %s" % (tuple(lr.shape), tuple(hr.shape)))
    if lr.dtype != torch.float32 or hr.dtype != torch.float32 or mask.dtype not in (torch.bool, torch.uint8) or recipe.dtype != torch.int32:
        raise ValueError("augment_batch: lr / hr must be float32, mask bool or uint8, recipe int32; got %s %s %s %s"
                         % (lr.dtype, hr.dtype, mask.dtype, recipe.dtype))
    if recipe.shape[1] != 3 + lr.shape[3]:
        raise ValueError("augment_batch: a recipe row is {i, f, k, perm[%d]} for the %d frames of lr; recipe has %d columns" % (lr.shape[3], lr.shape[3], recipe.shape[1]))
    if lr.shape[0] < 1:
        raise ValueError("augment_batch: empty base set")


@torch.library.custom_op("probav::augment_batch", mutates_args=(), device_types="cuda")
@_plain
def augment_batch(lr: Tensor, hr: Tensor, mask: Tensor, recipe: Tensor) -> tuple[Tensor, Tensor, Tensor]:
    """(lr_b [B, H, H, T, C], hr_b [B, S, S, 1], mask_b [B, S, S, 1]): out[b] = rot90(flip(x[i][:, :, perm] if LR else x[i], FL[f]), k) for
    recipe[b] = {i, f, k, perm}: one launch for the three tensors.  The kernel skips a row it could not apply without reading outside the base
    arrays; callers validate recipes on the host (augment.DeviceDataset does)."""
    _augment_args(lr, hr, mask, recipe, True)
    lr, hr, mask, recipe = _dense(lr, True), _dense(hr, True), _dense(mask, True), _dense(recipe)     # (csrc/augment_part.h: aug_aligned16 picks the path)
    B = recipe.shape[0]
    lr_b = torch.empty((B,) + tuple(lr.shape[1:]), dtype=lr.dtype, device=lr.device)
    hr_b = torch.empty((B,) + tuple(hr.shape[1:]), dtype=hr.dtype, device=lr.device)
    mask_b = torch.empty((B,) + tuple(mask.shape[1:]), dtype=mask.dtype, device=lr.device)
    if B:
        _lib.check(_lib.lib().probav_augment_batch(_lib.ptr(lr), _lib.ptr(hr), _lib.ptr(mask), lr.shape[0], lr.shape[1], lr.shape[3], lr.shape[4],
                                                   hr.shape[1], _lib.ptr(recipe), B, _lib.ptr(lr_b), _lib.ptr(hr_b), _lib.ptr(mask_b),
                                                   _lib.current_stream()), "probav_augment_batch")
    return lr_b, hr_b, mask_b


@augment_batch.register_fake
def _(lr, hr, mask, recipe):
    _augment_args(lr, hr, mask, recipe)
    B = recipe.shape[0]
    return lr.new_empty((B,) + tuple(lr.shape[1:])), hr.new_empty((B,) + tuple(hr.shape[1:])), mask.new_empty((B,) + tuple(mask.shape[1:]))


# ---------------------------------------------------------------------------------------------------------------------------------
# test-time self-ensemble (csrc/kernels_ensemble.hip; the variant tables and the definition are in ensemble.py).  No autograd: inference.
# lr [N, H, H, T, C] fp32; recipe [N V, 3 + T] int32 rows {i, f, k, perm}, row n V + v = variant v of patch n; sr [N V, S, S] or [N V, S, S, 1].
# ---------------------------------------------------------------------------------------------------------------------------------
ENSEMBLE_MAX_V = 256          # members are integers in [0, 2**16]: 256 of them sum to at most 2**24, exactly, in fp32 in any order


def _expand_args(lr, recipe, real=False):
    _operands("ensemble_expand", real, ("lr", lr, _F32, None), ("recipe", recipe, _I32, None))
    if lr.dim() != 5 or recipe.dim() != 2 or lr.shape[1] != lr.shape[2]:
        raise ValueError("ensemble_expand: lr [N, H, H, T, C] (square: a quarter turn needs it), recipe [B, 3 + T]; got %s %s"
                         % (tuple(lr.shape), tuple(recipe.shape)))
    if lr.dtype != torch.float32 or recipe.dtype != torch.int32:
        raise ValueError("ensemble_expand: lr must be float32, recipe int32; got %s %s" % (lr.dtype, recipe.dtype))
    if recipe.shape[1] != 3 + lr.shape[3]:
        raise ValueError("ensemble_expand: a recipe row is {i, f, k, perm[%d]} for the %d frames of lr; recipe has %d columns" % (lr.shape[3], lr.shape[3], recipe.shape[1]))
    if lr.shape[0] < 1:
        raise ValueError("ensemble_expand: no patches")


@torch.library.custom_op("probav::ensemble_expand", mutates_args=(), device_types="cuda")
@_plain
def ensemble_expand(lr: Tensor, recipe: Tensor) -> Tensor:
    """[B, H, H, T, C]: out[b] = rot90(flip(lr[i][:, :, perm], FL[f]), k) for recipe[b] = {i, f, k, perm} -- augment_batch's LR tensor alone.
    The kernel skips a row it could not apply without reading outside `lr`; callers validate recipes on the host (ensemble.py does)."""
    _expand_args(lr, recipe, True)
    lr, recipe = _dense(lr, True), _dense(recipe)
    B = recipe.shape[0]
    out = torch.empty((B,) + tuple(lr.shape[1:]), dtype=lr.dtype, device=lr.device)
    if B:
        _lib.check(_lib.lib().probav_ensemble_expand(_lib.ptr(lr), lr.shape[0], lr.shape[1], lr.shape[3], lr.shape[4], _lib.ptr(recipe), B,
                                                     _lib.ptr(out), _lib.current_stream()), "probav_ensemble_expand")
    return out


@ensemble_expand.register_fake
def _(lr, recipe):
    _expand_args(lr, recipe)
    return lr.new_empty((recipe.shape[0],) + tuple(lr.shape[1:]))


def _reduce_args(sr, recipe, V, sets, grid, real=False, lo=0.0, hi=0.0):
    """-> (N, S) after the checks the real and the fake kernel share."""
    _operands("ensemble_reduce", real, ("sr", sr, _F32, None), ("recipe", recipe, _I32, None))
    _want("ensemble_reduce", lo <= hi, "lo = %r, hi = %r: lo <= hi, neither a NaN", lo, hi)
    if sr.dim() == 4 and sr.shape[3] == 1:
        sr = sr[..., 0]
    if sr.dim() != 3 or sr.shape[1] != sr.shape[2] or recipe.dim() != 2 or recipe.shape[1] < 4:
        raise ValueError("ensemble_reduce: sr [N V, S, S] (or [N V, S, S, 1]), recipe [N V, 3 + T]; got %s %s" % (tuple(sr.shape), tuple(recipe.shape)))
    if sr.dtype != torch.float32 or recipe.dtype != torch.int32:
        raise ValueError("ensemble_reduce: sr must be float32, recipe int32; got %s %s" % (sr.dtype, recipe.dtype))
    if not 1 <= V <= ENSEMBLE_MAX_V:
        raise ValueError("ensemble_reduce: V = %d members; 1 <= V <= %d (each member is an integer up to 2**16: %d of them sum exactly in fp32, "
                         "more need not)" % (V, ENSEMBLE_MAX_V, ENSEMBLE_MAX_V))
    if sr.shape[0] < V or sr.shape[0] % V or recipe.shape[0] != sr.shape[0]:
        raise ValueError("ensemble_reduce: the %d predictions of sr and %d recipe rows do not make whole groups of V = %d" % (sr.shape[0], recipe.shape[0], V))
    N = sr.shape[0] // V
    if (grid == 0) != (sets == 0) or grid < 0 or sets < 0 or (grid and sets * grid * grid != N):
        raise ValueError("ensemble_reduce: sets = grid = 0 for patches, or sets * grid * grid == N = %d for stitched images; got sets %d, grid %d"
                         % (N, sets, grid))
    return N, sr.shape[1]


@torch.library.custom_op("probav::ensemble_reduce", mutates_args=(), device_types="cuda")
@_plain
def ensemble_reduce(sr: Tensor, recipe: Tensor, V: int, lo: float, hi: float, final_round: bool, sets: int, grid: int) -> Tensor:
    """mean over v < V of flip(rot90(rint(clip(sr[n V + v], lo, hi)), -k_v), FL[f_v]) -- exact fp32 sum, one correctly rounded division, rounded
    half to even once more if `final_round` -> [N, S, S] (sets = grid = 0) or the stitched [sets, grid S, grid S] of testClass.stitch_device."""
    N, S = _reduce_args(sr, recipe, V, sets, grid, True, lo, hi)
    sr, recipe = _dense(sr, True), _dense(recipe)
    out = torch.empty((sets, grid * S, grid * S) if grid else (N, S, S), dtype=torch.float32, device=sr.device)
    _lib.check(_lib.lib().probav_ensemble_reduce(_lib.ptr(sr), _lib.ptr(recipe), N, V, recipe.shape[1] - 3, S, lo, hi, 1 if final_round else 0, grid,
                                                 _lib.ptr(out), _lib.current_stream()), "probav_ensemble_reduce")
    return out


@ensemble_reduce.register_fake
def _(sr, recipe, V, lo, hi, final_round, sets, grid):
    N, S = _reduce_args(sr, recipe, V, sets, grid, False, lo, hi)
    return sr.new_empty((sets, grid * S, grid * S) if grid else (N, S, S), dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# overlapped-tile inference (csrc/kernels_tile.hip; the definition and the numpy statement are in tiles.py).  No autograd: inference.
# sr [n_images n n, S, S] or [..., S, S, 1] fp32: the tiles of every image in row-major order; w [S] int32, every entry in [1, 1024].
# ---------------------------------------------------------------------------------------------------------------------------------
def _tile_blend_args(sr, w, n_images, n, hr_stride, lo, hi, real=False):
    """-> (S, G) after the checks the real and the fake kernel share."""
    _operands("tile_blend", real, ("sr", sr, _F32, None), ("w", w, _I32, None))
    if sr.dim() == 4 and sr.shape[3] == 1:
        sr = sr[..., 0]
    if sr.dim() != 3 or sr.shape[1] != sr.shape[2] or w.dim() != 1:
        raise ValueError("tile_blend: sr [n_images n n, S, S] (or [..., S, S, 1]), w [S]; got %s %s" % (tuple(sr.shape), tuple(w.shape)))
    if sr.dtype != torch.float32 or w.dtype != torch.int32:
        raise ValueError("tile_blend: sr must be float32, w int32; got %s %s" % (sr.dtype, w.dtype))
    S = sr.shape[1]
    if n_images < 1 or n < 1 or S < 1 or sr.shape[0] != n_images * n * n or w.shape[0] != S:
        raise ValueError("tile_blend: the %d predictions of side %d in sr and a window w of %d do not make %d images of %d x %d tiles"
                         % (sr.shape[0], S, w.shape[0], n_images, n, n))
    if not 1 <= hr_stride <= S:
        raise ValueError("tile_blend: hr_stride = %d; 1 <= hr_stride <= S = %d (a gap between tiles would leave pixels without a weight)" % (hr_stride, S))
    if not lo <= hi:
        raise ValueError("tile_blend: lo = %r > hi = %r" % (lo, hi))
    return S, (n - 1) * hr_stride + S


@torch.library.custom_op("probav::tile_blend", mutates_args=(), device_types="cuda")
@_plain
def tile_blend(sr: Tensor, w: Tensor, n_images: int, n: int, hr_stride: int, lo: float, hi: float) -> Tensor:
    """out[y, x] = (sum_t W2 p_t) / (sum_t W2) over the tiles that cover (y, x), rounded half to even in exact 64-bit integer arithmetic;
    p = rint(clip(sr, lo, hi)), W2[i, j] = w[i] w[j], tile (a, c) at (a hr_stride, c hr_stride) -> [n_images, G, G], G = (n - 1) hr_stride + S.
    The window must hold integers in [1, 1024] (tiles.validate_window: callers check it on the host before the upload)."""
    S, G = _tile_blend_args(sr, w, n_images, n, hr_stride, lo, hi, True)
    sr, w = _dense(sr, True), _dense(w)
    out = torch.empty((n_images, G, G), dtype=torch.float32, device=sr.device)
    _lib.check(_lib.lib().probav_tile_blend(_lib.ptr(sr), _lib.ptr(w), n_images, n, S, hr_stride, lo, hi, _lib.ptr(out), _lib.current_stream()),
               "probav_tile_blend")
    return out


@tile_blend.register_fake
def _(sr, w, n_images, n, hr_stride, lo, hi):
    S, G = _tile_blend_args(sr, w, n_images, n, hr_stride, lo, hi)
    return sr.new_empty((n_images, G, G), dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# frame-window ensemble (csrc/kernels_windows.hip; the definition and the numpy statements are in frame_windows.py).  No autograd: inference.
# patches [N, T_pre, win, win] fp32 and counts [N, T_pre] int32: the builder's unfold of N tiles; sr [N W, S, S] or [..., S, S, 1] fp32.
# ---------------------------------------------------------------------------------------------------------------------------------
WINDOW_MODES = ("clear", "uniform")        # index = PROBAV_WINDOWS_CLEAR / PROBAV_WINDOWS_UNIFORM
WINDOWS_MAX = 64                           # W, and T_pre (one lane of the ranking wave per frame)
WINDOWS_LDS_BYTES = 160 * 1024 - 1040      # the staged tile: T_pre planes of _windows_plane_stride(win^2) floats beside the kernel's tables


def _windows_plane_stride(px):
    """The LDS plane stride of the gather kernel (csrc/kernels_windows.hip, fw_plane_stride)."""
    while px % 32 in (0, 1, 8, 11, 16, 21, 24, 31):
        px += 1
    return px


def _windows_gather_args(patches, counts, k, limit, windows, step, mode, real=False):
    """-> (N, T_pre, win) after the checks the real and the fake kernel share."""
    _operands("frame_windows_gather", real, ("patches", patches, _F32, None), ("counts", counts, _I32, None))
    if patches.dim() != 4 or counts.dim() != 2 or patches.shape[2] != patches.shape[3] or tuple(counts.shape) != tuple(patches.shape[:2]):
        raise ValueError("frame_windows_gather: patches [N, T_pre, win, win], counts [N, T_pre]; got %s %s" % (tuple(patches.shape), tuple(counts.shape)))
    if patches.dtype != torch.float32 or counts.dtype != torch.int32:
        raise ValueError("frame_windows_gather: patches must be float32, counts int32; got %s %s" % (patches.dtype, counts.dtype))
    if mode not in WINDOW_MODES:
        raise ValueError("frame_windows_gather: mode must be one of %r, got %r" % (WINDOW_MODES, mode))
    N, T_pre, win = patches.shape[0], patches.shape[1], patches.shape[2]
    if N < 1 or win < 1 or not 1 <= T_pre <= WINDOWS_MAX or not 1 <= windows <= WINDOWS_MAX or not 1 <= k <= WINDOWS_MAX or step < 1:
        raise ValueError("frame_windows_gather: patches / counts hold N = %d tiles of %d frames, k = %d, %d windows at step %d; N, step >= 1, 1 <= T_pre, k, windows <= %d"
                         % (N, T_pre, k, windows, step, WINDOWS_MAX))
    if windows > 1 and (windows - 1) * step + k > T_pre:
        raise ValueError("frame_windows_gather: (windows - 1) * step + k = %d frames, the pool has T_pre = %d" % ((windows - 1) * step + k, T_pre))
    if not 0 <= limit <= win * win + 1:
        raise ValueError("frame_windows_gather: limit = %d outside 0 .. win^2 + 1 = %d" % (limit, win * win + 1))
    if T_pre * win * win > 40960 or 4 * T_pre * _windows_plane_stride(win * win) > WINDOWS_LDS_BYTES:
        raise ValueError("frame_windows_gather: a tile of %d frames of %d x %d does not fit the 160 KiB of LDS it is staged in (at most 40960 floats, "
                         "each frame padded by up to 3)" % (T_pre, win, win))
    return N, T_pre, win


@torch.library.custom_op("probav::frame_windows_gather", mutates_args=(), device_types="cuda")
@_plain
def frame_windows_gather(patches: Tensor, counts: Tensor, k: int, limit: int, windows: int, step: int, mode: str) -> tuple[Tensor, Tensor, Tensor]:
    """(x [N, W, win, win, k, 1] fp32, weight [N, W] int32, sel [N, W, k] int32): per tile the frames with counts < limit (all when none)
    ordered by (count, index), tiled to at least k as the dataset builder tiles them, window j taking k of them from position j step on;
    x holds the chosen frames bit for bit with the frame index innermost, weight the clear pixels of every window's frames ("clear") or 1
    ("uniform"), all 1 where all are 0 -- frame_windows.frame_windows_select_numpy + _gather_numpy."""
    N, T_pre, win = _windows_gather_args(patches, counts, k, limit, windows, step, mode, True)
    patches, counts = _dense(patches, True), _dense(counts)
    x = torch.empty((N, windows, win, win, k, 1), dtype=torch.float32, device=patches.device)
    weight = torch.empty((N, windows), dtype=torch.int32, device=patches.device)
    sel = torch.empty((N, windows, k), dtype=torch.int32, device=patches.device)
    _lib.check(_lib.lib().probav_frame_windows_gather(_lib.ptr(patches), _lib.ptr(counts), N, T_pre, win, k, limit, windows, step, WINDOW_MODES.index(mode),
                                                      _lib.ptr(x), _lib.ptr(weight), _lib.ptr(sel), _lib.current_stream()), "probav_frame_windows_gather")
    return x, weight, sel


@frame_windows_gather.register_fake
def _(patches, counts, k, limit, windows, step, mode):
    N, T_pre, win = _windows_gather_args(patches, counts, k, limit, windows, step, mode)
    return (patches.new_empty((N, windows, win, win, k, 1), dtype=torch.float32), patches.new_empty((N, windows), dtype=torch.int32),
            patches.new_empty((N, windows, k), dtype=torch.int32))


def _windows_reduce_args(sr, weight, lo, hi, real=False):
    """-> (N, W, S) after the checks the real and the fake kernel share."""
    _operands("frame_windows_reduce", real, ("sr", sr, _F32, None), ("weight", weight, _I32, None))
    if sr.dim() == 4 and sr.shape[3] == 1:
        sr = sr[..., 0]
    if sr.dim() != 3 or sr.shape[1] != sr.shape[2] or weight.dim() != 2:
        raise ValueError("frame_windows_reduce: sr [N W, S, S] (or [..., S, S, 1]), weight [N, W]; got %s %s" % (tuple(sr.shape), tuple(weight.shape)))
    if sr.dtype != torch.float32 or weight.dtype != torch.int32:
        raise ValueError("frame_windows_reduce: sr must be float32, weight int32; got %s %s" % (sr.dtype, weight.dtype))
    N, W, S = weight.shape[0], weight.shape[1], sr.shape[1]
    if N < 1 or S < 1 or not 1 <= W <= WINDOWS_MAX or sr.shape[0] != N * W:
        raise ValueError("frame_windows_reduce: the %d predictions of side %d in sr do not make the %d tiles of %d windows of weight (1 <= W <= %d)"
                         % (sr.shape[0], S, N, W, WINDOWS_MAX))
    if not lo <= hi:
        raise ValueError("frame_windows_reduce: lo = %r > hi = %r" % (lo, hi))
    return N, W, S


@torch.library.custom_op("probav::frame_windows_reduce", mutates_args=(), device_types="cuda")
@_plain
def frame_windows_reduce(sr: Tensor, weight: Tensor, lo: float, hi: float) -> Tensor:
    """out[n] = (sum_j weight[n, j] p[n W + j]) / (sum_j weight[n, j]) rounded half to even in exact 64-bit integer arithmetic,
    p = rint(clip(sr, lo, hi)) -> [N, S, S] fp32 holding integers -- frame_windows.frame_windows_reduce_numpy.  The weights must be
    non-negative with a positive sum per tile (what frame_windows_gather writes)."""
    N, W, S = _windows_reduce_args(sr, weight, lo, hi, True)
    sr, weight = _dense(sr, True), _dense(weight)
    out = torch.empty((N, S, S), dtype=torch.float32, device=sr.device)
    _lib.check(_lib.lib().probav_frame_windows_reduce(_lib.ptr(sr), _lib.ptr(weight), N, W, S, lo, hi, _lib.ptr(out), _lib.current_stream()),
               "probav_frame_windows_reduce")
    return out


@frame_windows_reduce.register_fake
def _(sr, weight, lo, hi):
    N, W, S = _windows_reduce_args(sr, weight, lo, hi)
    return sr.new_empty((N, S, S), dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# bicubic-mean baseline (csrc/kernels_baseline.hip; the definition and the numpy statement are in baseline.py).  No autograd: a yardstick.
# frames [F, H, W] uint16 (int16 is taken as the same bits), clear [F, H, W] bool or uint8 (nonzero = clear), set_offsets [S + 1] int64.
# ---------------------------------------------------------------------------------------------------------------------------------
BASELINE_MODES = ("esa", "clear")          # index = PROBAV_BASELINE_ESA / PROBAV_BASELINE_CLEAR


def _baseline_args(frames, clear, set_offsets, mode, real=False):
    """-> (S, H, W) after the checks the real and the fake kernel share."""
    _operands("baseline_upscale_mean", real, ("frames", frames, _U16, None), ("clear", clear, _MASK, None), ("set_offsets", set_offsets, _I64, None))
    if frames.dim() != 3 or clear.shape != frames.shape or set_offsets.dim() != 1 or set_offsets.shape[0] < 2:
        raise ValueError("baseline_upscale_mean: frames, clear [F, H, W], set_offsets [S + 1]; got %s %s %s"
                         % (tuple(frames.shape), tuple(clear.shape), tuple(set_offsets.shape)))
    if frames.dtype not in (torch.uint16, torch.int16) or clear.dtype not in (torch.bool, torch.uint8) or set_offsets.dtype != torch.int64:
        raise ValueError("baseline_upscale_mean: frames must be uint16 (or int16 bits), clear bool or uint8, set_offsets int64; got %s %s %s"
                         % (frames.dtype, clear.dtype, set_offsets.dtype))
    if mode not in BASELINE_MODES:
        raise ValueError("baseline_upscale_mean: mode must be one of %r, got %r" % (BASELINE_MODES, mode))
    if frames.shape[0] < 1 or frames.shape[1] < 1 or frames.shape[2] < 1:
        raise ValueError("baseline_upscale_mean: no frames, or frames without pixels: %s" % (tuple(frames.shape),))
    return set_offsets.shape[0] - 1, frames.shape[1], frames.shape[2]


@torch.library.custom_op("probav::baseline_upscale_mean", mutates_args=(), device_types="cuda")
@_plain
def baseline_upscale_mean(frames: Tensor, clear: Tensor, set_offsets: Tensor, mode: str) -> tuple[Tensor, Tensor]:
    """(out [S, 3H, 3W] fp32 holding integers, k_used [S] int32): every frame upscaled 3 x by the Keys cubic in integers over 729, the frames
    `mode` chooses summed in int64, divided by 729 K with one rounding half to even, clipped to [0, 65535] -- baseline.baseline_numpy, bit for bit.
    The sets must satisfy the preconditions of include/probav_hip.h (baseline.baseline_device checks them on the host before the upload); a set
    that breaks them gets k_used = -1 and its image is left unwritten."""
    S, H, W = _baseline_args(frames, clear, set_offsets, mode, True)
    frames, clear, set_offsets = _dense(frames), _dense(clear), _dense(set_offsets)
    out = torch.empty((S, 3 * H, 3 * W), dtype=torch.float32, device=frames.device)
    k_used = torch.empty((S,), dtype=torch.int32, device=frames.device)
    counts = torch.empty((frames.shape[0],), dtype=torch.int32, device=frames.device)
    _lib.check(_lib.lib().probav_baseline_upscale_mean(_lib.ptr(frames), _lib.ptr(clear), _lib.ptr(set_offsets), S, frames.shape[0], H, W, 3,
                                                       BASELINE_MODES.index(mode), _lib.ptr(counts), _lib.ptr(out), _lib.ptr(k_used),
                                                       _lib.current_stream()), "probav_baseline_upscale_mean")
    return out, k_used


@baseline_upscale_mean.register_fake
def _(frames, clear, set_offsets, mode):
    S, H, W = _baseline_args(frames, clear, set_offsets, mode)
    return frames.new_empty((S, 3 * H, 3 * W), dtype=torch.float32), frames.new_empty((S,), dtype=torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# random crops (csrc/kernels_crops.hip; the definition, the numpy statements and the recipes are in crops.py).  No autograd: they move
# and count input bits.
# ---------------------------------------------------------------------------------------------------------------------------------
CROPS_LDS_BYTES = 160 * 1024
CROPS_STATIC_LDS = 768             # the crop kernel's counts and frame list


def _window_counts_args(masks, pad, win, stride, real=False):
    """-> (M, H, W, ny, nx) after the checks the real and the fake kernel share."""
    _operands("window_counts", real, ("masks", masks, _MASK, None))
    if masks.dim() != 3 or masks.dtype not in (torch.uint8, torch.bool):
        raise ValueError("window_counts: masks [M, H, W] uint8 or bool; got %s %s" % (tuple(masks.shape), masks.dtype))
    M, H, W = masks.shape
    if M < 1 or not 1 <= H <= 32767 or not 1 <= W <= 32767 or not 0 <= pad < min(H, W) or not 1 <= win <= min(1024, H + 2 * pad, W + 2 * pad) \
            or not 1 <= stride <= 1024:
        raise ValueError("window_counts: %d masks of %d x %d, pad %d, win %d, stride %d; M >= 1, 1 <= H, W <= 32767, 0 <= pad < min(H, W), "
                         "1 <= win <= min(1024, H + 2 pad, W + 2 pad), 1 <= stride <= 1024" % (M, H, W, pad, win, stride))
    if 64 * (W + 2 * pad) > CROPS_LDS_BYTES:
        raise ValueError("window_counts: 16 rows of column sums of %d padded columns do not fit the 160 KiB of LDS" % (W + 2 * pad))
    return M, H, W, (H + 2 * pad - win) // stride + 1, (W + 2 * pad - win) // stride + 1


@torch.library.custom_op("probav::window_counts", mutates_args=(), device_types="cuda")
@_plain
def window_counts(masks: Tensor, pad: int, win: int, stride: int) -> Tensor:
    """int32 [M, ny, nx]: the nonzero pixels of every win x win window at `stride` of masks [M, H, W] reflect-padded by `pad`
    (crops.window_counts_numpy), exact."""
    M, H, W, ny, nx = _window_counts_args(masks, pad, win, stride, True)
    masks = _dense(masks)
    out = torch.empty((M, ny, nx), dtype=torch.int32, device=masks.device)
    _lib.check(_lib.lib().probav_window_counts(_lib.ptr(masks), M, H, W, pad, win, stride, _lib.ptr(out), _lib.current_stream()), "probav_window_counts")
    return out


@window_counts.register_fake
def _(masks, pad, win, stride):
    M, _, _, ny, nx = _window_counts_args(masks, pad, win, stride)
    return masks.new_empty((M, ny, nx), dtype=torch.int32)


def _crop_batch_args(lr, lr_mask, hr, hr_clear, positions, recipe, P, pad, win, scale, limit, real=False):
    """-> (S, T_pre, H, k, B, side) after the checks the real and the fake kernel share (side = scale P, the HR window's)."""
    _operands("crop_batch", real, ("lr", lr, _F32, None), ("lr_mask", lr_mask, _MASK, None), ("hr", hr, _F32, None), ("hr_clear", hr_clear, _MASK, None),
              ("positions", positions, _I32, None), ("recipe", recipe, _I32, None))
    if lr.dim() != 4 or lr.shape[2] != lr.shape[3] or tuple(lr_mask.shape) != tuple(lr.shape) or hr.dim() != 3 or tuple(hr_clear.shape) != tuple(hr.shape) \
            or positions.dim() != 2 or positions.shape[1] != 3 or recipe.dim() != 2:
        raise ValueError("crop_batch: lr / lr_mask [S, T_pre, H, H], hr / hr_clear [S, r H, r H], positions [V, 3], recipe [B, 3 + k]; got %s %s %s %s %s %s"
                         % tuple(tuple(t.shape) for t in (lr, lr_mask, hr, hr_clear, positions, recipe)))
    if lr.dtype != torch.float32 or hr.dtype != torch.float32 or lr_mask.dtype not in (torch.uint8, torch.bool) \
            or hr_clear.dtype not in (torch.uint8, torch.bool) or positions.dtype != torch.int32 or recipe.dtype != torch.int32:
        raise ValueError("crop_batch: lr / hr must be float32, lr_mask / hr_clear uint8 or bool, positions / recipe int32; got %s %s %s %s %s %s"
                         % (lr.dtype, lr_mask.dtype, hr.dtype, hr_clear.dtype, positions.dtype, recipe.dtype))
    S, T_pre, H = lr.shape[0], lr.shape[1], lr.shape[2]
    k, B = recipe.shape[1] - 3, recipe.shape[0]
    if S < 1 or positions.shape[0] < 1 or not 1 <= T_pre <= WINDOWS_MAX or not 1 <= k <= WINDOWS_MAX:
        raise ValueError("crop_batch: lr holds %d scenes of %d frames, positions %d rows, recipe gives k = %d; S, V >= 1, 1 <= T_pre, k <= %d"
                         % (S, T_pre, positions.shape[0], k, WINDOWS_MAX))
    if not 1 <= P <= H <= 32767 or not 0 <= pad < H or not P <= win <= min(P + 2 * pad, 1024) or not 1 <= scale <= 64 or scale * P > 1024:
        raise ValueError("crop_batch: H = %d, P = %d, pad = %d, win = %d, scale = %d; 1 <= P <= H, 0 <= pad < H, P <= win <= min(P + 2 pad, 1024), "
                         "1 <= scale <= 64, scale P <= 1024" % (H, P, pad, win, scale))
    if hr.shape[0] != S or hr.shape[1] != scale * H or hr.shape[2] != scale * H:
        raise ValueError("crop_batch: hr must be [%d, %d, %d] for scale %d; got %s" % (S, scale * H, scale * H, scale, tuple(hr.shape)))
    if not 0 <= limit <= win * win + 1:
        raise ValueError("crop_batch: limit = %d outside 0 .. win^2 + 1 = %d" % (limit, win * win + 1))
    side = scale * P
    rnd = lambda b: (b + 15) & ~15
    if max(rnd(4 * win * win * k) + 4 * win * k, rnd(4 * side * side) + 4 * side) + CROPS_STATIC_LDS > CROPS_LDS_BYTES:
        raise ValueError("crop_batch: one sample (k = %d LR windows of %d x %d, or an HR window of %d x %d floats) does not fit the 160 KiB of LDS it is "
                         "staged in" % (k, win, win, side, side))
    return S, T_pre, H, k, B, side


@torch.library.custom_op("probav::crop_batch", mutates_args=(), device_types="cuda")
@_plain
def crop_batch(lr: Tensor, lr_mask: Tensor, hr: Tensor, hr_clear: Tensor, positions: Tensor, recipe: Tensor, P: int, pad: int, win: int, scale: int,
               limit: int) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """(lr_b [B, win, win, k, 1] fp32, hr_b [B, rP, rP, 1] fp32, mask_b [B, rP, rP, 1] in hr_clear's dtype, sel [B, k] int32): the training samples
    of recipe rows {j, f, q, perm}, cut at positions[j] = {scene, y, x} out of the resident scenes, their k frames chosen per window as the
    dataset builder chooses them (counts < limit, (count, index) order, tiled) -- crops.crop_batch_numpy.  One launch.  The kernel skips a row
    it could not apply without reading outside the arrays; callers validate recipes on the host (crops.CropDataset does)."""
    S, T_pre, H, k, B, side = _crop_batch_args(lr, lr_mask, hr, hr_clear, positions, recipe, P, pad, win, scale, limit, True)
    lr, lr_mask, hr, hr_clear, positions, recipe = (_dense(t) for t in (lr, lr_mask, hr, hr_clear, positions, recipe))
    lr_b = torch.empty((B, win, win, k, 1), dtype=torch.float32, device=lr.device)
    hr_b = torch.empty((B, side, side, 1), dtype=torch.float32, device=lr.device)
    mask_b = torch.empty((B, side, side, 1), dtype=hr_clear.dtype, device=lr.device)
    sel = torch.empty((B, k), dtype=torch.int32, device=lr.device)
    if B:
        _lib.check(_lib.lib().probav_crop_batch(_lib.ptr(lr), _lib.ptr(lr_mask), _lib.ptr(hr), _lib.ptr(hr_clear), S, T_pre, H, P, pad, win, scale, k, limit,
                                                _lib.ptr(positions), positions.shape[0], _lib.ptr(recipe), B, _lib.ptr(lr_b), _lib.ptr(hr_b),
                                                _lib.ptr(mask_b), _lib.ptr(sel), _lib.current_stream()), "probav_crop_batch")
    return lr_b, hr_b, mask_b, sel


@crop_batch.register_fake
def _(lr, lr_mask, hr, hr_clear, positions, recipe, P, pad, win, scale, limit):
    _, _, _, k, B, side = _crop_batch_args(lr, lr_mask, hr, hr_clear, positions, recipe, P, pad, win, scale, limit)
    return (lr.new_empty((B, win, win, k, 1)), hr.new_empty((B, side, side, 1)), hr_clear.new_empty((B, side, side, 1)),
            recipe.new_empty((B, k), dtype=torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------------
# per-layer operators (SURVEY.md section 8b's minimum op set): what the engine is made of, as torch ops of their own, so that a variant
# network (another block order, an iWDSR-style head) can be composed from them.  Each has its autograd formula registered in terms of
# the other ops of the set; the whole-network op above stays the fast path (one workspace, fused scales, side stream).
# Layouts are the reference's: activations [N, H, W, T, C] (channels last), filters in Keras layout [kh, kw, kt, Cin, Cout].
# ---------------------------------------------------------------------------------------------------------------------------------
import ctypes as _ct


def _geom17(N, hwt, cin, out_hwt, cout, k, pad, reflect, relu):
    return (_ct.c_int32 * 17)(N, hwt[0], hwt[1], hwt[2], cin, out_hwt[0], out_hwt[1], out_hwt[2], cout, k[0], k[1], k[2], pad[0], pad[1], pad[2],
                              1 if reflect else 0, 1 if relu else 0)


def _conv_out(x, w, pad):
    k = tuple(int(d) for d in w.shape[:3])
    out = tuple(int(x.shape[1 + i]) + 2 * pad[i] - k[i] + 1 for i in range(3))
    return k, out


def _conv_scalars(op, ksize, pad, impl, kname):
    _want(op, len(ksize) == 3 and all(int(k) >= 1 for k in ksize), "%s must give three positive kernel extents [kh, kw, kt], got %s", kname, list(ksize))
    _want(op, len(pad) == 3 and all(0 <= int(pad[i]) <= int(ksize[i]) - 1 for i in range(3)),
          "pad must be three values [ph, pw, pt] in 0 .. k - 1 for the kernel %s, got %s", list(ksize), list(pad))
    _want(op, 0 <= impl <= 4, "impl = %d; the kernel families are 0 .. 4", impl)


def _conv_fwd_args(real, x, w, bias, pad, skip, gate, impl):
    """-> (k, out) after the checks the real and the fake implementation share."""
    op = "conv3d_k3_fwd"
    _operands(op, real, ("x", x, _F32, 5), ("w", w, _F32, 5), ("bias", bias, _F32, 1), ("skip", skip, _F32, 5), ("gate", gate, _F32, 5))
    _conv_scalars(op, tuple(w.shape[:3]), pad, impl, "w")
    k, out = _conv_out(x, w, pad)
    _want(op, x.shape[0] >= 1, "x holds an empty batch, got shape %s (the network ops refuse one)", tuple(x.shape))
    _want(op, w.shape[3] == x.shape[4] and w.shape[3] >= 1 and w.shape[4] >= 1, "w %s takes %d input channels, x %s has %d",
          tuple(w.shape), w.shape[3], tuple(x.shape), x.shape[4])
    _want(op, min(out) >= 1, "x %s under w %s with pad %s leaves no output: %s", tuple(x.shape), tuple(w.shape), list(pad), out)
    _want(op, bias.numel() == w.shape[4], "bias holds %d values, w %s has %d output channels", bias.numel(), tuple(w.shape), w.shape[4])
    yshape = (int(x.shape[0]),) + out + (int(w.shape[4]),)
    _want(op, skip is None or tuple(skip.shape) == yshape, "skip must have the output's shape %s, got %s", yshape, None if skip is None else tuple(skip.shape))
    _want(op, gate is None or tuple(gate.shape) == tuple(x.shape), "gate must have x's shape %s, got %s", tuple(x.shape), None if gate is None else tuple(gate.shape))
    return k, out


@torch.library.custom_op("probav::conv3d_k3_fwd", mutates_args=(), device_types="cuda")
@_plain
def conv3d_k3_fwd(x: Tensor, w: Tensor, bias: Tensor, pad: list[int], reflect_hw: bool, relu: bool, skip: Optional[Tensor] = None,
                  gate: Optional[Tensor] = None, impl: int = 4) -> Tensor:
    """y = act(conv(x * [gate > 0], w) + bias) + skip: Conv3D of models/modelsTF.py:168-183,187-203 (`same`: pad 1, `valid`: pad 0; reflect_hw: the
    tf.pad(REFLECT) of the height / width axes in front of convReducer_1) -- and, with flipped taps and swapped channels, its backward-data."""
    k, out = _conv_fwd_args(True, x, w, bias, pad, skip, gate, impl)
    x, w, bias, skip, gate = _dense(x), _dense(w), _dense(bias), _dense(skip), _dense(gate)
    y = torch.empty((x.shape[0],) + out + (w.shape[4],), dtype=torch.float32, device=x.device)
    g = _geom17(x.shape[0], x.shape[1:4], x.shape[4], out, w.shape[4], k, pad, reflect_hw, relu)
    rc = _lib.lib().probav_conv3d_forward(_ct.byref(g), _lib.ptr(x), _lib.ptr(gate), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(skip), _lib.ptr(y), impl,
                                          _lib.current_stream())
    if rc == _lib.PROBAV_EINVAL and impl != 0:             # a geometry this MFMA family does not cover: the shape-agnostic kernels, as the engine does
        rc = _lib.lib().probav_conv3d_forward(_ct.byref(g), _lib.ptr(x), _lib.ptr(gate), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(skip), _lib.ptr(y), 0,
                                              _lib.current_stream())
    _lib.check(rc, "probav_conv3d_forward")
    return y


@conv3d_k3_fwd.register_fake
def _(x, w, bias, pad, reflect_hw, relu, skip=None, gate=None, impl=4):
    k, out = _conv_fwd_args(False, x, w, bias, pad, skip, gate, impl)
    return x.new_empty((x.shape[0],) + out + (w.shape[4],), dtype=torch.float32)


def _conv_wgrad_args(real, x, dy, ksize, pad, gate, impl):
    op = "conv3d_k3_bwd_weight"
    _operands(op, real, ("x", x, _F32, 5), ("dy", dy, _F32, 5), ("gate", gate, _F32, 5))
    _conv_scalars(op, ksize, pad, impl, "ksize")
    _want(op, x.shape[0] >= 1 and x.shape[4] >= 1 and dy.shape[4] >= 1, "x %s or dy %s is empty (the network ops refuse an empty batch)", tuple(x.shape), tuple(dy.shape))
    want = (int(x.shape[0]),) + tuple(int(x.shape[1 + i]) + 2 * int(pad[i]) - int(ksize[i]) + 1 for i in range(3))
    _want(op, tuple(dy.shape[:4]) == want and min(want) >= 1, "dy must be %s + (Cout,) for x %s, kernel %s, pad %s; got %s",
          want, tuple(x.shape), list(ksize), list(pad), tuple(dy.shape))
    _want(op, gate is None or tuple(gate.shape) == tuple(dy.shape), "gate (the layer's own output) must have dy's shape %s, got %s",
          tuple(dy.shape), None if gate is None else tuple(gate.shape))


@torch.library.custom_op("probav::conv3d_k3_bwd_weight", mutates_args=(), device_types="cuda")
@_plain
def conv3d_k3_bwd_weight(x: Tensor, dy: Tensor, ksize: list[int], pad: list[int], reflect_hw: bool, gate: Optional[Tensor] = None,
                         impl: int = 4) -> tuple[Tensor, Tensor]:
    """(dw [kh, kw, kt, Cin, Cout], db [Cout]) of the same layer from its input and the gradient of its output (gate: the layer's own
    post-ReLU output, when it has one)."""
    _conv_wgrad_args(True, x, dy, ksize, pad, gate, impl)
    x, dy, gate = _dense(x), _dense(dy), _dense(gate)
    out = tuple(int(dy.shape[1 + i]) for i in range(3))
    g = _geom17(x.shape[0], x.shape[1:4], x.shape[4], out, dy.shape[4], ksize, pad, reflect_hw, gate is not None)
    L = _lib.lib()
    use = impl
    nbytes = L.probav_conv3d_wgrad_scratch_bytes(_ct.byref(g), use)
    if nbytes == 0 and use != 0:
        use = 0
        nbytes = L.probav_conv3d_wgrad_scratch_bytes(_ct.byref(g), 0)
    scratch = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device=x.device)
    dw = torch.empty(tuple(ksize) + (x.shape[4], dy.shape[4]), dtype=torch.float32, device=x.device)
    db = torch.empty((dy.shape[4],), dtype=torch.float32, device=x.device)
    _lib.check(L.probav_conv3d_wgrad(_ct.byref(g), _lib.ptr(x), _lib.ptr(dy), _lib.ptr(gate), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(scratch), nbytes, use,
                                     _lib.current_stream()), "probav_conv3d_wgrad")
    return dw, db


@conv3d_k3_bwd_weight.register_fake
def _(x, dy, ksize, pad, reflect_hw, gate=None, impl=4):
    _conv_wgrad_args(False, x, dy, ksize, pad, gate, impl)
    return x.new_empty(tuple(ksize) + (x.shape[4], dy.shape[4]), dtype=torch.float32), x.new_empty((dy.shape[4],), dtype=torch.float32)


def _conv_setup(ctx, inputs, output):
    x, w, bias, pad, reflect_hw, relu, skip, gate, impl = inputs
    if gate is not None:
        raise RuntimeError("probav::conv3d_k3_fwd: the `gate` form is the backward-data operator of another layer and has no autograd formula")
    ctx.save_for_backward(x, w, output if relu else None)
    ctx.pad, ctx.reflect_hw, ctx.relu, ctx.impl, ctx.has_skip = list(pad), reflect_hw, relu, impl, skip is not None


def _conv_bwd(ctx, dy):
    x, w, y = ctx.saved_tensors
    dy = dy.contiguous().float()
    k = tuple(w.shape[:3])
    gate = None
    if ctx.relu:                                            # y = relu(z) + skip: the gate is z > 0; with a skip the saved output no longer shows it
        if ctx.has_skip:
            raise RuntimeError("probav::conv3d_k3_fwd: relu together with skip has no autograd formula (the network never combines them on one layer)")
        gate = y
    dw, db = torch.ops.probav.conv3d_k3_bwd_weight(x, dy, list(k), ctx.pad, ctx.reflect_hw, gate, ctx.impl)
    dx = None
    if ctx.needs_input_grad[0]:
        if ctx.reflect_hw:
            raise RuntimeError("probav::conv3d_k3_fwd: the input gradient of a reflect-padded layer goes through the engine (fold of the mirrored border)")
        wT = torch.flip(w, dims=(0, 1, 2)).transpose(3, 4).contiguous()                 # flipped taps, swapped channels
        bpad = [k[i] - 1 - ctx.pad[i] for i in range(3)]                                 # "full" correlation minus the forward padding
        zero = torch.zeros(w.shape[3], dtype=torch.float32, device=x.device)
        dx = torch.ops.probav.conv3d_k3_fwd(dy, wT, zero, bpad, False, False, None, gate, ctx.impl)
    return dx, dw, db, None, None, None, (dy if ctx.has_skip else None), None, None


conv3d_k3_fwd.register_autograd(_conv_bwd, setup_context=_conv_setup)


PW_CIN, PW_HIDDEN, PW_MAX_D = 32, 256, 26 # the fused pair's fixed widths (csrc/kernels_x6.hip): expConv_i 32 -> 256, decConv_i 256 -> D


def _pw_args(op, real, x, w1, b1, w2, b2, vox_per_sample, impl, d_dec=None, d_skip=None):
    """-> (voxels, D) after the checks the real and the fake implementation of the pointwise pair share."""
    _operands(op, real, ("x", x, _F32, None), ("w1", w1, _F32, 2), ("b1", b1, _F32, 1), ("w2", w2, _F32, 2), ("b2", b2, _F32, 1),
              ("d_dec", d_dec, _F32, None), ("d_skip", d_skip, _F32, None))
    _want(op, x.dim() >= 1 and x.shape[-1] == PW_CIN, "x must be [..., %d], got %s", PW_CIN, tuple(x.shape))
    D = int(w2.shape[1])
    _want(op, tuple(w1.shape) == (PW_CIN, PW_HIDDEN) and b1.numel() == PW_HIDDEN and w2.shape[0] == PW_HIDDEN and D >= 1,
          "w1 [%d, %d], b1 [%d], w2 [%d, D]; got %s %s %s", PW_CIN, PW_HIDDEN, PW_HIDDEN, PW_HIDDEN, tuple(w1.shape), tuple(b1.shape), tuple(w2.shape))
    _want(op, b2 is None or b2.numel() == D, "b2 holds %d values, w2 %s has %d output channels", 0 if b2 is None else b2.numel(), tuple(w2.shape), D)
    nvox = x.numel() // PW_CIN
    _want(op, nvox >= 1, "x holds no voxel, got shape %s (the network ops refuse an empty batch)", tuple(x.shape))
    _want(op, D <= PW_MAX_D, "w2 %s has %d output channels, the fused pair takes at most %d", tuple(w2.shape), D, PW_MAX_D)
    _want(op, vox_per_sample >= 0 and (vox_per_sample == 0 or nvox % vox_per_sample == 0) and 0 <= impl <= 4,
          "vox_per_sample = %d must be 0 or divide the %d voxels of x, and impl = %d lie in 0 .. 4", vox_per_sample, nvox, impl)
    _want(op, d_dec is None or tuple(d_dec.shape) == tuple(x.shape[:-1]) + (D,), "d_dec must be %s, got %s", tuple(x.shape[:-1]) + (D,),
          None if d_dec is None else tuple(d_dec.shape))
    _want(op, d_skip is None or tuple(d_skip.shape) == tuple(x.shape), "d_skip must have x's shape %s, got %s", tuple(x.shape),
          None if d_skip is None else tuple(d_skip.shape))
    return nvox, D


@torch.library.custom_op("probav::pw_expand_relu_decay_fwd", mutates_args=(), device_types="cuda")
@_plain
def pw_expand_relu_decay_fwd(x: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, vox_per_sample: int = 0, impl: int = 4) -> Tensor:
    """expConv_i (1x1x1, 32 -> 256) + ReLU + decConv_i (1x1x1, 256 -> D), fused: models/modelsTF.py:179-183.  x [..., 32] -> [..., D]; the
    256-channel tensor never reaches memory.  vox_per_sample: voxels of one patch (the unit the H3 arithmetic scales by; 0 = one sample)."""
    nvox, D = _pw_args("pw_expand_relu_decay_fwd", True, x, w1, b1, w2, b2, vox_per_sample, impl)
    x, w1, b1, w2, b2 = _dense(x), _dense(w1), _dense(b1), _dense(w2), _dense(b2)
    dec = torch.empty(tuple(x.shape[:-1]) + (D,), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().probav_pw_forward(_lib.ptr(x), _lib.ptr(w1), _lib.ptr(b1), _lib.ptr(w2), _lib.ptr(b2), _lib.ptr(dec), nvox, vox_per_sample,
                                            w2.shape[-1], impl, _lib.current_stream()), "probav_pw_forward")
    return dec


@pw_expand_relu_decay_fwd.register_fake
def _(x, w1, b1, w2, b2, vox_per_sample=0, impl=4):
    _pw_args("pw_expand_relu_decay_fwd", False, x, w1, b1, w2, b2, vox_per_sample, impl)
    return x.new_empty(tuple(x.shape[:-1]) + (w2.shape[-1],), dtype=torch.float32)


@torch.library.custom_op("probav::pw_expand_relu_decay_bwd", mutates_args=(), device_types="cuda")
@_plain
def pw_expand_relu_decay_bwd(x: Tensor, d_dec: Tensor, d_skip: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, vox_per_sample: int = 0,
                             impl: int = 4) -> tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """The fused reverse pass: (dx = d_skip + dL/dx, dw1, db1, dw2, db2); the hidden tile is recomputed, never stored."""
    nvox, D = _pw_args("pw_expand_relu_decay_bwd", True, x, w1, b1, w2, None, vox_per_sample, impl, d_dec, d_skip)
    x, d_dec, d_skip, w1, b1, w2 = _dense(x), _dense(d_dec), _dense(d_skip), _dense(w1), _dense(b1), _dense(w2)
    L = _lib.lib()
    nbytes = L.probav_pw_backward_scratch_bytes(D)
    scratch = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    dw1, db1, dw2, db2 = torch.empty_like(w1), torch.empty_like(b1), torch.empty_like(w2), torch.empty((D,), dtype=torch.float32, device=x.device)
    _lib.check(L.probav_pw_backward(_lib.ptr(x), _lib.ptr(d_dec), _lib.ptr(d_skip), _lib.ptr(w1), _lib.ptr(b1), _lib.ptr(w2), _lib.ptr(dx), _lib.ptr(dw1),
                                    _lib.ptr(db1), _lib.ptr(dw2), _lib.ptr(db2), _lib.ptr(scratch), nbytes, nvox, vox_per_sample, D, impl,
                                    _lib.current_stream()), "probav_pw_backward")
    return dx, dw1, db1, dw2, db2


@pw_expand_relu_decay_bwd.register_fake
def _(x, d_dec, d_skip, w1, b1, w2, vox_per_sample=0, impl=4):
    _pw_args("pw_expand_relu_decay_bwd", False, x, w1, b1, w2, None, vox_per_sample, impl, d_dec, d_skip)
    c = torch.contiguous_format
    return (torch.empty_like(x, memory_format=c), torch.empty_like(w1, memory_format=c), torch.empty_like(b1, memory_format=c),
            torch.empty_like(w2, memory_format=c), x.new_empty((w2.shape[-1],), dtype=torch.float32))


def _pw_setup(ctx, inputs, output):
    x, w1, b1, w2, b2, vps, impl = inputs
    ctx.save_for_backward(x, w1, b1, w2)
    ctx.vps, ctx.impl = vps, impl


def _pw_bwd(ctx, d_dec):
    x, w1, b1, w2 = ctx.saved_tensors
    d_dec = d_dec.contiguous().float()
    dx, dw1, db1, dw2, db2 = torch.ops.probav.pw_expand_relu_decay_bwd(x, d_dec, torch.zeros_like(x), w1, b1, w2, ctx.vps, ctx.impl)
    return dx, dw1, db1, dw2, db2, None, None


pw_expand_relu_decay_fwd.register_autograd(_pw_bwd, setup_context=_pw_setup)


def _wn_args(op, real, flat, engine, dweff=None, inv_norm=None):
    """-> (param_count, weff_count, cout_total) after the checks both implementations share.  The outputs are sized by the engine, so the fake
    rule asks it too (as it always has): a trace of these two ops needs a live handle."""
    _operands(op, real, ("flat", flat, _F32, None), ("dweff", dweff, _F32, None), ("inv_norm", inv_norm, _F32, None))
    nparams, nw, nc = engine_sizes(engine)[:3]
    _want(op, flat.numel() == nparams, "flat holds %d values, the engine has %d parameters", flat.numel(), nparams)
    _want(op, dweff is None or dweff.numel() == nw, "dweff holds %d values, the engine's effective weights %d", 0 if dweff is None else dweff.numel(), nw)
    _want(op, inv_norm is None or inv_norm.numel() == nc, "inv_norm holds %d values, the engine has %d output channels",
          0 if inv_norm is None else inv_norm.numel(), nc)
    return nparams, nw, nc


@torch.library.custom_op("probav::wn_weight_fwd", mutates_args=(), device_types="cuda")
@_plain
def wn_weight_fwd(flat: Tensor, engine: int) -> tuple[Tensor, Tensor, Tensor]:
    """TFA WeightNormalization of every layer of the engine's flat parameter buffer (w = g v / ||v||, per output channel):
    -> (weff: layers in order, Keras layout; weffT: flipped taps / swapped channels for the backward-data operators; inv_norm per output channel)."""
    nparams, nw, nc = _wn_args("wn_weight_fwd", True, flat, engine)
    flat = _dense(flat)
    L, h = _lib.lib(), c_void_p(engine)
    weff, weffT = torch.empty(nw, dtype=torch.float32, device=flat.device), torch.empty(nw, dtype=torch.float32, device=flat.device)
    inv = torch.empty(nc, dtype=torch.float32, device=flat.device)
    _lib.check(L.probav_wn_forward(h, _lib.ptr(flat), _lib.ptr(weff), _lib.ptr(weffT), _lib.ptr(inv), _lib.current_stream()), "probav_wn_forward")
    return weff, weffT, inv


@wn_weight_fwd.register_fake
def _(flat, engine):
    nparams, nw, nc = _wn_args("wn_weight_fwd", False, flat, engine)
    return flat.new_empty((nw,)), flat.new_empty((nw,)), flat.new_empty((nc,))


@torch.library.custom_op("probav::wn_weight_bwd", mutates_args=(), device_types="cuda")
@_plain
def wn_weight_bwd(flat: Tensor, dweff: Tensor, inv_norm: Tensor, engine: int) -> Tensor:
    """Gradient of the flat parameter buffer (g, v of every layer; the bias slots are left to the caller) from the gradient of `weff`."""
    _wn_args("wn_weight_bwd", True, flat, engine, dweff, inv_norm)
    flat, dweff, inv_norm = _dense(flat), _dense(dweff), _dense(inv_norm)
    grads = torch.zeros_like(flat)
    _lib.check(_lib.lib().probav_wn_backward(c_void_p(engine), _lib.ptr(flat), _lib.ptr(dweff), _lib.ptr(inv_norm), _lib.ptr(grads), _lib.current_stream()),
               "probav_wn_backward")
    return grads


@wn_weight_bwd.register_fake
def _(flat, dweff, inv_norm, engine):
    _wn_args("wn_weight_bwd", False, flat, engine, dweff, inv_norm)
    return torch.empty_like(flat, memory_format=torch.contiguous_format)


def _wn_setup(ctx, inputs, output):
    flat, engine = inputs
    ctx.save_for_backward(flat, output[2])
    ctx.engine = engine
    ctx.mark_non_differentiable(output[1], output[2])
    ctx.set_materialize_grads(False)


def _wn_bwd(ctx, dweff, dweffT, dinv):
    if dweff is None:
        return None, None
    flat, inv = ctx.saved_tensors
    return torch.ops.probav.wn_weight_bwd(flat, dweff.contiguous().float(), inv, ctx.engine), None


wn_weight_fwd.register_autograd(_wn_bwd, setup_context=_wn_setup)


# ---------------------------------------------------------------------------------------------------------------------------------
# FuseNet (csrc/kernels_fusenet.hip; the statement: fusenet_numpy.py)
# ---------------------------------------------------------------------------------------------------------------------------------
FUSENET_PARAMS = 48 * 48 * 64 + 3 * 64
FUSENET_NO_DX = ("FuseNet computes no gradient for its input: the stitched image is data (d loss / d x is out of scope); "
                 "pass an input that does not require grad")


def _fusenet_args(op, real, x, flat, g=None, y=None, stats=None):
    """-> (B, H, W) after the checks the real and the fake implementation share."""
    _operands(op, real, ("x", x, _F32, 3), ("flat", flat, _F32, None), ("g", g, _F32, None),
              ("y", y, _F32, None), ("stats", stats, _F32, None))
    if flat.numel() != FUSENET_PARAMS:
        raise ValueError("%s: flat must hold %d values (kernel, bias, gamma, beta), got %d" % (op, FUSENET_PARAMS, flat.numel()))
    B, H, W = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    _want(op, B >= 1 and H >= 1 and W >= 1, "x holds an empty batch or image, got shape %s (the network ops refuse one)", tuple(x.shape))
    if g is not None and (tuple(g.shape) != (B, H, W) or tuple(y.shape) != (B, H, W, 64) or tuple(stats.shape) != (B, 64, 2)):
        raise ValueError("%s: g %s, y %s, stats %s do not belong to x %s" % (op, tuple(g.shape), tuple(y.shape), tuple(stats.shape), tuple(x.shape)))
    return B, H, W


def _fusenet_ws(B, H, W, backward, device):
    n = _lib.lib().probav_fusenet_workspace_bytes(B, H, W, backward)
    if n == 0:
        raise ValueError("fusenet: unsupported shape B=%d H=%d W=%d (all >= 1, B <= 65535, H, W <= 32768, 64 B H W < 2^31)" % (B, H, W))
    return torch.empty((n + 7) // 8, dtype=torch.float64, device=device)


@torch.library.custom_op("probav::fusenet_forward", mutates_args=(), device_types="cuda")
@_plain
def fusenet_forward(x: Tensor, flat: Tensor, residual: bool) -> tuple[Tensor, Tensor, Tensor]:
    """-> (out [B, H, W] = x + m, or the branch m alone with residual=False; y [B, H, W, 64], the convolution without its bias; stats [B, 64, 2] =
    (mu, 1 / sqrt(var + 1e-3))).  y and stats are what the reverse pass reads: outputs, like the residuals of any differentiable op."""
    B, H, W = _fusenet_args("fusenet_forward", True, x, flat)
    x, flat = _dense(x), _dense(flat)
    out = torch.empty((B, H, W), dtype=torch.float32, device=x.device)
    y = torch.empty((B, H, W, 64), dtype=torch.float32, device=x.device)
    stats = torch.empty((B, 64, 2), dtype=torch.float32, device=x.device)
    ws = _fusenet_ws(B, H, W, 0, x.device)
    _lib.check(_lib.lib().probav_fusenet_forward(_lib.ptr(x), _lib.ptr(flat), flat.numel(), B, H, W, 1 if residual else 0, _lib.ptr(out), _lib.ptr(y),
                                                 _lib.ptr(stats), _lib.ptr(ws), ws.numel() * 8, _lib.current_stream()), "probav_fusenet_forward")
    return out, y, stats


@fusenet_forward.register_fake
def _(x, flat, residual):
    B, H, W = _fusenet_args("fusenet_forward", False, x, flat)
    return x.new_empty((B, H, W), dtype=torch.float32), x.new_empty((B, H, W, 64), dtype=torch.float32), x.new_empty((B, 64, 2), dtype=torch.float32)


@torch.library.custom_op("probav::fusenet_backward", mutates_args=(), device_types="cuda")
@_plain
def fusenet_backward(g: Tensor, x: Tensor, y: Tensor, stats: Tensor, flat: Tensor) -> Tensor:
    """d loss / d flat from g = d loss / d out; x, y, stats, flat as the matching forward took and returned them, only READ here (functional:
    the scratch is this call's own).  The bias slots are exact zeros."""
    B, H, W = _fusenet_args("fusenet_backward", True, x, flat, g, y, stats)
    g, x, y, stats, flat = (_dense(t) for t in (g, x, y, stats, flat))
    dflat = torch.empty(FUSENET_PARAMS, dtype=torch.float32, device=x.device)
    ws = _fusenet_ws(B, H, W, 1, x.device)
    _lib.check(_lib.lib().probav_fusenet_backward(_lib.ptr(g), _lib.ptr(x), _lib.ptr(y), _lib.ptr(stats), _lib.ptr(flat), flat.numel(), B, H, W, _lib.ptr(dflat),
                                                  _lib.ptr(ws), ws.numel() * 8, _lib.current_stream()), "probav_fusenet_backward")
    return dflat.view(flat.shape)


@fusenet_backward.register_fake
def _(g, x, y, stats, flat):
    _fusenet_args("fusenet_backward", False, x, flat, g, y, stats)
    return torch.empty_like(flat, memory_format=torch.contiguous_format)


def _fusenet_setup(ctx, inputs, output):
    x, flat, residual = inputs
    ctx.save_for_backward(x, flat, output[1], output[2])
    ctx.mark_non_differentiable(output[1], output[2])
    ctx.set_materialize_grads(False)


def _fusenet_bwd(ctx, g, dy, dstats):
    if ctx.needs_input_grad[0]:
        raise RuntimeError(FUSENET_NO_DX)
    if g is None:
        return None, None, None
    x, flat, y, stats = ctx.saved_tensors
    return None, torch.ops.probav.fusenet_backward(g.contiguous().float(), x, y, stats, flat), None


fusenet_forward.register_autograd(_fusenet_bwd, setup_context=_fusenet_setup)
