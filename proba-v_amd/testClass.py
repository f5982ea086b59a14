"""Host-side mirror of the reference's inference wrappers: models/testClass.py::Enhancer and the helpers of
test.py (``resolve``, ``resolveByBatch``, ``evaluate``, ``reconstruct_from_patches``; test.py:103-160).

Patch-wise evaluation is kept exactly as the reference does it -- the network is NOT run on the whole
frame, because its 'same'-padded convolutions see zeros beyond each 22x22 patch.
The forward pass, the clip to [0, 2**16] and the round-half-even run on the device (HIP kernels);
only the stitched uint16-range image returns to the host.
"""
import numpy as np
import torch

from . import _lib, ops            # noqa: F401  (ops registers torch.ops.probav.*)
from .ensemble import EnsembleSpec, ensemble_reduce_numpy, validate_ensemble_recipe      # noqa: F401  (re-exported)
from . import tiles as _tiles
from .tiles import TileSpec, tile_blend_numpy      # noqa: F401  (re-exported)
from .frame_windows import FrameWindowSpec         # noqa: F401  (re-exported)


def _device_of(model):
    return next(model.parameters()).device


def _require_hip(model, what):
    """The model's device; RuntimeError unless it is a HIP device (`what`: "the self-ensemble runs as HIP kernels", ...)."""
    dev = _device_of(model)
    if dev.type != "cuda":
        raise RuntimeError("the model lives on %s: %s on a gfx950 device (no CPU fallback)" % (dev, what))
    return dev


def _host_images(imgs):
    """Device images [n, G, G] -> the list of [G, G, 1] float64 arrays the reference's `evaluate` returns: one copy back."""
    return [im[:, :, None] for im in imgs.cpu().numpy().astype(np.float64)]


def resolve_device(model, lr_batch):
    """test.py:114-122 without the final host copy: float32 cast -> model -> clip_by_value(0, 2**16) -> round."""
    dev = _device_of(model)
    x = torch.as_tensor(np.ascontiguousarray(lr_batch) if isinstance(lr_batch, np.ndarray) else lr_batch)
    x = x.to(device=dev, dtype=torch.float32)
    with torch.no_grad():
        sr = model(x, training=False)
        out = torch.ops.probav.clip_round(sr, 0.0, float(2 ** 16))
    return out


def resolve(model, lr_batch):
    """test.py:114-122 -> numpy float32 [b, 3P, 3P, 1]."""
    return resolve_device(model, lr_batch).cpu().numpy()


LAUNCH_BATCH = 2048        # patches per launch set of the coalesced paths (5.0 GB of workspace at T = 9)


def _whole_micro_batches(launch_batch, micro_batch):
    """Patches per launch set: the whole micro-batches that fit `launch_batch`, at least one."""
    return max(1, launch_batch // max(1, micro_batch)) * max(1, micro_batch)


def _is_engine_model(model):
    return hasattr(model, "_handle") and hasattr(model, "flat")


def resolveByBatch(model, lr_batch, batch_size=16):
    """test.py:125-134: micro-batches of `batch_size` plus the remainder, concatenated.

    The reference slices because its GPU could not hold more; the slices are invisible in the result (they are concatenated in order, and the
    network has no cross-sample term: models/modelsTF.py:15-43).  On the engine every kernel family is bitwise independent of the batch
    (tests/test_gpu_h3_range.py::test_forward_is_bitwise_independent_of_the_batch, tests/test_gpu_parity.py::test_config4_*), so the
    micro-batches are coalesced into launch sets of up to LAUNCH_BATCH patches and the result is the same array, bit for bit, at the
    batched rate (a 16-patch launch set fills a sixteenth of the device).  Any other callable takes the reference's loop as written
    (tests/test_ref_plumbing.py holds its call pattern to the reference's own function)."""
    if _is_engine_model(model) and resolve is _RESOLVE:
        return resolve_coalesced(model, lr_batch, batch_size).cpu().numpy()
    n, rem = divmod(lr_batch.shape[0], batch_size)
    cache = [resolve(model, lr_batch[batch_size * i: batch_size * (i + 1)]) for i in range(n)]
    if rem:
        cache.append(resolve(model, lr_batch[batch_size * n: batch_size * n + rem]))
    return np.concatenate(cache)


_RESOLVE = resolve


def resolve_coalesced(model, lr_batch, batch_size=16, launch_batch=None):
    """`resolveByBatch` on the device: the reference's micro-batches of `batch_size` grouped into launch sets of whole micro-batches
    (at most `launch_batch` patches, default LAUNCH_BATCH); returns the device tensor [n, 3P, 3P, 1]."""
    launch_batch = LAUNCH_BATCH if launch_batch is None else launch_batch
    per = _whole_micro_batches(launch_batch, batch_size)
    n = lr_batch.shape[0]
    outs = [resolve_device(model, lr_batch[i:i + per]) for i in range(0, n, per)]
    return outs[0] if len(outs) == 1 else torch.cat(outs)


def resolveBySampleAveraging(model, lr_batch, rng=None):
    """test.py:137-146: the mean over 20 predictions, each on a cumulative random permutation of the LR frames (axis 3); every
    prediction is clipped and rounded (it goes through `resolve`) before the mean.  `rng`: numpy Generator (the reference draws
    from the global numpy state).  Returns a device tensor [b, 3P, 3P, 1]."""
    rng = np.random.default_rng() if rng is None else rng
    x = torch.as_tensor(np.ascontiguousarray(lr_batch) if isinstance(lr_batch, np.ndarray) else lr_batch).to(_device_of(model))
    acc = None
    for _ in range(20):
        idx = torch.as_tensor(rng.permutation(x.shape[3])).to(x.device)
        x = x.index_select(3, idx)                            # the permutations compound, as in the reference
        sr = resolve_device(model, x.contiguous())
        acc = sr.double() if acc is None else acc + sr.double()
    return (acc / 20.0).float()


def _ensemble_launch_sets(model, flat, spec, final, launch_batch, grid=0):
    """The ensemble of `flat` [N, H, H, T, C] in launch sets of max(1, launch_batch // V) WHOLE base patches (the members of one patch are
    never split, and the forward workspace is no larger than the plain path's): expand -> the engine's forward -> reduce, all on the
    device.  grid = g: launch sets are whole images of g * g patches and every yielded tensor is [images, g S, g S]; grid = 0: [n, S, S]."""
    if final not in ("mean", "round"):
        raise ValueError("final must be 'mean' or 'round', got %r" % (final,))
    dev = _require_hip(model, "the self-ensemble runs as HIP kernels")
    N, T, V = flat.shape[0], flat.shape[3], spec.V
    per = max(1, (LAUNCH_BATCH if launch_batch is None else launch_batch) // V)
    if grid:
        per -= per % (grid * grid)
    recipe = spec.recipe(min(per, N), T)
    validate_ensemble_recipe(recipe, min(per, N), V, T)
    rec = torch.from_numpy(recipe).to(dev)
    for i in range(0, N, per):
        x = torch.as_tensor(flat[i:i + per]).to(device=dev, dtype=torch.float32)
        r = rec[:x.shape[0] * V]
        with torch.no_grad():
            sr = model(torch.ops.probav.ensemble_expand(x, r), training=False)
            out = torch.ops.probav.ensemble_reduce(sr, r, V, 0.0, float(2 ** 16), final == "round", x.shape[0] // (grid * grid) if grid else 0, grid)
        yield out


def resolve_ensemble(model, lr_batch, spec, final="mean", launch_batch=None):
    """The self-ensemble prediction of every patch of `lr_batch` [b, H, H, T, C] (ensemble.py states it): the mean over the spec's V variants
    of the clipped, rounded prediction of each, turned back -- test.py:137-146's sample averaging with flips and quarter turns beside the
    frame orders, reproducible from the spec.  final = "mean": the fp32 mean, as the reference's helper returns it; "round": rounded half
    to even once more (the uint16-range form).  Returns a device tensor [b, 3P, 3P, 1]."""
    flat = np.ascontiguousarray(lr_batch) if isinstance(lr_batch, np.ndarray) else lr_batch
    outs = list(_ensemble_launch_sets(model, flat, spec, final, launch_batch))
    return (outs[0] if len(outs) == 1 else torch.cat(outs)).unsqueeze(-1)


def reconstruct_from_patches(images):
    """test.py:149-160: row-major n x n stitch of square patches into a [384, 384, 1] image
    (float64 zeros, like np.zeros in the reference)."""
    rec = np.zeros((384, 384, 1))
    n = int(len(images) ** 0.5)
    ps = images.shape[1]
    k = 0
    for i in range(n):
        for j in range(n):
            rec[i * ps:(i + 1) * ps, j * ps:(j + 1) * ps] = images[k]
            k += 1
    return rec.reshape((384, 384, 1))


def evaluate(model, X_test_patches, batch_size=16):
    """test.py:103-111: one stitched prediction per image set.  On the engine the image sets and their micro-batches are coalesced
    (see `resolveByBatch`): same pixels, one copy back."""
    if _is_engine_model(model) and resolve is _RESOLVE:
        return evaluate_device(model, X_test_patches, micro_batch=batch_size)
    return [reconstruct_from_patches(resolveByBatch(model, X_test_patches[i], batch_size))
            for i in range(X_test_patches.shape[0])]


class Enhancer:
    """models/testClass.py:11-39 (unused by the reference's own test.py; kept for API parity,
    including its hard-coded 4 x 4 grid of 96-pixel blocks)."""

    def __init__(self, model, patchLR):
        self.model = model
        self.patchLR = patchLR

    def enhance(self):
        return [self.reconstruct(np.array(self.enhancePatch(s).cpu())) for s in self.patchLR]

    def enhancePatch(self, set):
        return resolve_device(self.model, set)

    def reconstruct(self, patches):
        img = np.zeros((384, 384, 1))
        k = 0
        for i in range(4):
            for j in range(4):
                img[i * 96:(i + 1) * 96, j * 96:(j + 1) * 96] = patches[k]
                k += 1
        return img.reshape((384, 384, 1))


# ---------------------------------------------------------------------------------------------------------------------
# Device-side image pipeline around the forward kernels.  Tensor re-arrangement only (torch plumbing);
# the arithmetic stays in the HIP engine and in probav_clip_round.
# ---------------------------------------------------------------------------------------------------------------------
def unfold_frames(frames, patchSizeLR=16, maxShift=6):
    """Registered LR frames [sets, T, H, W] (H = W = 128) -> patches [sets, n*n, P+s, P+s, T, 1] on the frames' device.

    Restates what the reference's offline preprocessing does before test.py sees the data
    (utils/dataGenerator.py:108-121: reflect-pad every frame by maxShift//2, then unfold (P+maxShift)-sized windows with
    stride P, row-major) followed by test.py:38's transpose to [sets, patch, H, W, T, C]."""
    import torch.nn.functional as F
    f = torch.as_tensor(frames)
    S, T, H, W = f.shape
    pad, win = maxShift // 2, patchSizeLR + maxShift
    fp = F.pad(f.reshape(S * T, 1, H, W).float(), (pad, pad, pad, pad), mode="reflect")
    u = fp.unfold(2, win, patchSizeLR).unfold(3, win, patchSizeLR)           # [S*T, 1, n, n, win, win]
    n = u.shape[2]
    u = u.reshape(S, T, n * n, win, win).permute(0, 2, 3, 4, 1).contiguous()  # [S, n*n, win, win, T]
    return u.unsqueeze(-1)


def stitch_device(sr, sets):
    """[sets*n*n, ps, ps, 1] -> [sets, n*ps, n*ps]: the row-major block layout of test.py:149-160, on the device."""
    nn_, ps = sr.shape[0] // sets, sr.shape[1]
    n = int(round(nn_ ** 0.5))
    return sr.reshape(sets, n, n, ps, ps).permute(0, 1, 3, 2, 4).reshape(sets, n * ps, n * ps)


def _predict_flat(model, flat, ensemble, launch_batch):
    """The predictions sr [n, S, S] (device tensor) of the flat batch `flat` [n, win, win, T, 1]: forward passes in launch sets of at most
    `launch_batch` inputs (default LAUNCH_BATCH), raw; with an `ensemble` in launch sets of launch_batch // V inputs through
    `resolve_ensemble`'s kernels, every prediction the rounded self-ensemble (final="round")."""
    dev = _device_of(model)
    S = model.scale * model.patchSizeLR
    sr = torch.empty((flat.shape[0], S, S), dtype=torch.float32, device=dev)
    if ensemble is not None:
        i = 0
        for out in _ensemble_launch_sets(model, flat, ensemble, "round", launch_batch):
            sr[i:i + out.shape[0]] = out
            i += out.shape[0]
    else:
        per = max(1, LAUNCH_BATCH if launch_batch is None else launch_batch)
        with torch.no_grad():
            for i in range(0, flat.shape[0], per):
                x = flat[i:i + per].to(device=dev, dtype=torch.float32)
                sr[i:i + x.shape[0]] = model(x, training=False)[..., 0]
    return sr


def resolve_tiled(model, tiles, spec, ensemble=None, launch_batch=None):
    """Overlapping tiles [images, n n, P+s, P+s, T, 1] (tiles.build_tiles at spec.stride; the chunk of images the caller chose) -> the blended
    uint16-range images [images, G, G] (device tensor), G = scale * ((n - 1) * stride + P): tiles.py states the blend.  The forward passes
    run in launch sets of at most `launch_batch` tiles (default LAUNCH_BATCH), with an `ensemble` (EnsembleSpec) in launch sets of
    launch_batch // V tiles through `resolve_ensemble`'s kernels, every tile rounded (final="round"); then ONE blend kernel, which clips and
    rounds the raw predictions itself.  Integer arithmetic from there on: the images do not depend on the launch sets."""
    dev = _require_hip(model, "the tile blend runs as a HIP kernel")
    t = torch.as_tensor(tiles)
    images, nn_ = t.shape[0], t.shape[1]
    n = int(round(nn_ ** 0.5))
    if t.dim() != 6 or n * n != nn_:
        raise ValueError("tiles must be [images, n * n, win, win, T, 1], got %s" % (tuple(t.shape),))
    P, r = model.patchSizeLR, model.scale
    if not 1 <= spec.stride <= P:
        raise ValueError("tile stride %d outside 1..%d" % (spec.stride, P))
    S = r * P
    w = torch.from_numpy(spec.weights(S)).to(dev)                    # validated on the host: every weight in [1, 1024]
    sr = _predict_flat(model, t.reshape((-1,) + tuple(t.shape[2:])), ensemble, launch_batch)
    return torch.ops.probav.tile_blend(sr, w, images, n, r * spec.stride, 0.0, float(2 ** 16))


def resolve_tiled_frames(model, imgsLR_masked, spec, config, ensemble=None, launch_batch=None, budget=None):
    """The registered LR frames of whole image sets (trimmedArrayDir/<TEST|TRAIN>imgLR_<band>.npy, masked [images, T_pre, 1, H, H]) -> the
    blended images [images, G, G] on the device: tiles.build_tiles + resolve_tiled in chunks of whole images sized so that neither the
    unfolded tiles nor the predictions of a chunk exceed `budget` bytes (default tiles.CHUNK_BYTES, 1 GiB each)."""
    H, T_pre = imgsLR_masked.shape[3], imgsLR_masked.shape[1]
    spec.validate(int(config["patch_size"]), H)
    per = _tiles.images_per_chunk(spec, config, H, T_pre, _tiles.CHUNK_BYTES if budget is None else budget)
    dev = _device_of(model)
    outs = []
    for i in range(0, imgsLR_masked.shape[0], per):
        t = _tiles.build_tiles(imgsLR_masked[i:i + per], spec, config, dev)
        outs.append(resolve_tiled(model, t, spec, ensemble=ensemble, launch_batch=launch_batch))
        del t
    return outs[0] if len(outs) == 1 else torch.cat(outs)


def evaluate_tiled_frames(model, imgsLR_masked, spec, config, ensemble=None, launch_batch=None, budget=None):
    """`resolve_tiled_frames` in the form `evaluate_device` returns: a list of [G, G, 1] float64 arrays, one copy back."""
    return _host_images(resolve_tiled_frames(model, imgsLR_masked, spec, config, ensemble=ensemble, launch_batch=launch_batch, budget=budget))


def resolve_windowed(model, patches, counts, wspec, tspec=None, ensemble=None, launch_batch=None):
    """The frame-window ensemble of one chunk of images (frame_windows.py states it).  patches [images, n n, T_pre, win, win] fp32 and counts
    [images, n n, T_pre] int32 are the builder's unfold at the tile stride (device tensors); `wspec` a FrameWindowSpec.  One gather kernel
    chooses the frames of every tile and writes the inputs of its W windows, the forward passes run over the flat [images n n W, win, win,
    k, 1] inputs in launch sets (with an `ensemble` through `resolve_ensemble`'s kernels, every window member rounded), one reduce kernel
    takes the weighted integer mean of the W members of every tile and `tile_blend` places the tiles: `tspec` (a TileSpec), or stride P with
    the box window, the plain stitch -> [images, G, G].  Integer arithmetic after each member's rint: the images do not depend on the
    launch sets."""
    dev = _require_hip(model, "the frame windows run as HIP kernels")
    if patches.dim() != 5 or counts.dim() != 3:
        raise ValueError("patches [images, n n, T_pre, win, win] and counts [images, n n, T_pre] expected, got %s %s" % (tuple(patches.shape), tuple(counts.shape)))
    images, nn_, T_pre, win = patches.shape[:4]
    n = int(round(nn_ ** 0.5))
    P, r, k = model.patchSizeLR, model.scale, model.numImgLR
    if n * n != nn_:
        raise ValueError("%d tiles per image do not make a square grid" % nn_)
    wspec.validate(T_pre, k)
    tspec = TileSpec(P, "box") if tspec is None else tspec
    if not 1 <= tspec.stride <= P:
        raise ValueError("tile stride %d outside 1..%d" % (tspec.stride, P))
    S = r * P
    w = torch.from_numpy(tspec.weights(S)).to(dev)
    x, weight, _ = torch.ops.probav.frame_windows_gather(patches.reshape(images * nn_, T_pre, win, win), counts.reshape(images * nn_, T_pre), k,
                                                         wspec.limit(win * win), wspec.windows, wspec.step, wspec.weights)
    sr = _predict_flat(model, x.reshape((-1,) + tuple(x.shape[2:])), ensemble, launch_batch)
    del x
    tiles_sr = torch.ops.probav.frame_windows_reduce(sr, weight, 0.0, float(2 ** 16))
    return torch.ops.probav.tile_blend(tiles_sr, w, images, n, r * tspec.stride, 0.0, float(2 ** 16))


def resolve_windowed_frames(model, imgsLR_masked, wspec, config, tiles=None, ensemble=None, launch_batch=None, budget=None):
    """The registered LR frames of whole image sets (trimmedArrayDir/<TEST|TRAIN>imgLR_<band>.npy, masked [images, T_pre, 1, H, H]) -> the
    frame-window images [images, G, G] on the device: the builder's unfold at the tile stride (`tiles`, a TileSpec; None: stride P, the
    plain stitch) + `resolve_windowed`, in chunks of whole images sized so that the unfolded tiles, the W-fold network inputs and the
    predictions of a chunk each stay under `budget` bytes (default tiles.CHUNK_BYTES).  No counts come to the host."""
    from . import frame_windows as _fw, prep
    S_, T_pre, C, H, W_ = imgsLR_masked.shape
    if C != 1 or H != W_:
        raise ValueError("square greyscale frames [images, T, 1, H, H] expected, got %s" % (imgsLR_masked.shape,))
    P, b, win, _, k, _ = _tiles.geometry(config)
    tspec = TileSpec(P, "box") if tiles is None else tiles
    tspec.validate(P, H)
    wspec = wspec.bind(config).validate(T_pre, k, config)
    per = _fw.images_per_chunk(wspec, tspec, config, H, T_pre, budget)
    outs = []
    for i in range(0, S_, per):
        chunk = imgsLR_masked[i:i + per]
        data = np.ma.getdata(chunk).reshape(-1, T_pre, H, H)
        mask = np.ma.getmaskarray(chunk).reshape(-1, T_pre, H, H)
        pt, _, pc = prep._device_patches(data, mask, b, win, tspec.stride)
        outs.append(resolve_windowed(model, pt, pc, wspec, tspec, ensemble=ensemble, launch_batch=launch_batch))
        del pt, pc
    return outs[0] if len(outs) == 1 else torch.cat(outs)


def evaluate_windowed_frames(model, imgsLR_masked, wspec, config, tiles=None, ensemble=None, launch_batch=None, budget=None):
    """`resolve_windowed_frames` in the form `evaluate_device` returns: a list of [G, G, 1] float64 arrays, one copy back."""
    return _host_images(resolve_windowed_frames(model, imgsLR_masked, wspec, config, tiles=tiles, ensemble=ensemble, launch_batch=launch_batch,
                                                budget=budget))


def resolve_images(model, patches, micro_batch=2048, launch_batch=None, ensemble=None, final="round", tiles=None):
    """All image sets at once: patches [sets, n*n, P+s, P+s, T, 1] -> uint16-range images [sets, 3nP, 3nP] (device tensor).
    Samples are independent in every kernel family (models/modelsTF.py:15-43 has no cross-sample term; the H3 kernels scale their
    operands per sample), so any micro-batch gives bit-identical pixels to the reference's batches of 16
    (tests/test_gpu_h3_range.py::test_forward_is_bitwise_independent_of_the_batch).
    `micro_batch` is the reference-visible slicing (test.py:125: 16); `launch_batch` is how many patches one launch set of the engine takes:
    None (default) coalesces whole micro-batches up to max(micro_batch, LAUNCH_BATCH); `launch_batch=micro_batch` launches every micro-batch
    on its own, as the reference's loop does (the parity tests compare the two bit for bit).
    `ensemble` (an EnsembleSpec; None = the plain path, untouched): every patch is predicted in the spec's V variants and the images are the
    self-ensemble of `resolve_ensemble` in the form `final` ("round" = uint16-range, what a PNG takes; "mean" = the fp32 mean).  A launch set
    then holds launch_batch // V whole patches -- whole images, reduced and stitched by one kernel, when that many fit; `micro_batch` plays
    no part.
    `tiles` (a TileSpec; None = the paths above, untouched): `patches` are the overlapping tiles of tiles.build_tiles at that stride and the
    images are their blend, `resolve_tiled` (always the rounded form; `micro_batch` plays no part)."""
    if tiles is not None:
        if final != "round":
            raise ValueError("blended tiles are integers: final must be 'round', got %r" % (final,))
        return resolve_tiled(model, patches, tiles, ensemble=ensemble, launch_batch=launch_batch)
    dev = _device_of(model)
    p = torch.as_tensor(patches)
    sets = p.shape[0]
    flat = p.reshape((-1,) + tuple(p.shape[2:]))
    if ensemble is not None:
        n = int(round(p.shape[1] ** 0.5))
        whole = n * n == p.shape[1] and (LAUNCH_BATCH if launch_batch is None else launch_batch) // ensemble.V >= n * n
        outs = list(_ensemble_launch_sets(model, flat, ensemble, final, launch_batch, grid=n if whole else 0))
        out = outs[0] if len(outs) == 1 else torch.cat(outs)
        return out if whole else stitch_device(out.unsqueeze(-1), sets)
    if launch_batch is None:
        launch_batch = max(micro_batch, LAUNCH_BATCH)
    per = _whole_micro_batches(launch_batch, micro_batch)
    outs = []
    for i in range(0, flat.shape[0], per):
        outs.append(resolve_device(model, flat[i:i + per].to(dev)))
    return stitch_device(torch.cat(outs) if len(outs) > 1 else outs[0], sets)


def evaluate_device(model, X_test_patches, micro_batch=2048, launch_batch=None, ensemble=None, final="round", tiles=None, windows=None, config=None):
    """test.py:103-111 through the device pipeline: every image set in micro-batches of `micro_batch` patches (16 = the reference's
    resolveByBatch; coalesced into launch sets unless `launch_batch` says otherwise), clip / round and the 8 x 8 stitch on the device, ONE
    copy back.  Returns a list of [384, 384, 1] float64 arrays, element for element what the reference's `evaluate` returns.
    `ensemble`, `final`: the self-ensemble of `resolve_images` instead of the plain prediction (None: today's path and bytes).
    `tiles`: a TileSpec when X_test_patches are overlapping tiles to be blended (`resolve_images`; None: today's path and bytes).
    `windows`: a FrameWindowSpec when X_test_patches are the registered frames of whole image sets (masked [images, T_pre, 1, H, H]) and the
    images are their frame-window ensemble, `evaluate_windowed_frames` with the parsed cfg `config` (`tiles` is then the tile grid of the
    frames; None: today's path and bytes)."""
    if windows is not None:
        if final != "round" or config is None:
            raise ValueError("frame windows give integers (final must be 'round', got %r) and take the parsed cfg as config=" % (final,))
        return evaluate_windowed_frames(model, X_test_patches, windows, config, tiles=tiles, ensemble=ensemble, launch_batch=launch_batch)
    return _host_images(resolve_images(model, X_test_patches, micro_batch=micro_batch, launch_batch=launch_batch, ensemble=ensemble, final=final,
                                       tiles=tiles))
