"""Host-side mirror of the reference's models/loss.py::Losses (shift-compensated L1 / L2 / cPSNR).

Argument order is the reference's: ``(patchHR, maskHR, predPatchHR)`` (models/loss.py:37,55,73).  One fused
HIP launch evaluates all (2*cropBorder+1)^2 candidate registrations of every sample and returns the
per-sample minima of the L1 and L2 terms, the cPSNR maximum and the arg-min shifts; the backward
launch differentiates the arg-min shift including the brightness-bias term.  Both are
torch custom ops (`torch.ops.probav.shift_loss` with its registered autograd formula, `probav.shift_metrics`), and so are the two other
losses a cfg can select (`probav.shift_l1edge_loss`, `probav.revssim_loss`): this module calls ops only.  The reference unrolls the same
work into ~600 TensorFlow ops per step (models/loss.py:79-81).
"""
import torch

from . import _lib, ops             # noqa: F401  (ops registers torch.ops.probav.*)


def _prep(patchHR, maskHR, predPatchHR):
    pred = _lib.require_device(predPatchHR, "predPatchHR")
    dev = pred.device
    hr = torch.as_tensor(patchHR).to(device=dev, dtype=torch.float32).contiguous()
    m = torch.as_tensor(maskHR).to(device=dev)
    m = (m if m.dtype == torch.bool else m != 0).contiguous().view(torch.uint8)   # True = clear pixel (train.py:43)
    pred = pred.contiguous().float()
    if hr.shape != pred.shape or m.shape != pred.shape or pred.dim() != 4 or pred.shape[3] != 1 or pred.shape[1] != pred.shape[2]:
        raise ValueError("expected patchHR, maskHR, predPatchHR all [B, S, S, 1]; got %s %s %s"
                         % (tuple(hr.shape), tuple(m.shape), tuple(pred.shape)))
    return hr, m, pred


# Largest crop (targetShape - 2 * cropBorder) of the two losses whose kernels hold the crop in LDS (include/probav_hip.h): 160 KiB of
# (3 L^2 + (L + 2)^2) floats for sobel_l1_mix, of (5 L + L^2) doubles for l1msssim.  Patch sizes 16, 24 and 32 (crops 42, 66, 90) fit both.
L1EDGE_MAX_CROP = 100
REVSSIM_MAX_CROP = 140


class Losses:
    """models/loss.py:8-35: all losses / metrics in one object; constants follow the reference.

    Where this differs from the reference, by decision (include/probav_hip.h, 'loss / metric'): among shifts that tie exactly the FIRST in
    shift order is selected and differentiated (tf.reduce_min splits the gradient equally among them); a shift under which a sample has no
    clear pixel is no candidate, and a sample without a clear pixel under any shift has NaN losses and cPSNR (arg 0)."""

    def __init__(self, targetShape=(96, 96, 1), cropBorder=3, bitDepth=16):
        self.targetShapeHeight, self.targetShapeWidth, self.targetShapeChannels = targetShape
        self.cropBorder = cropBorder
        self.maxPixelShift = 2 * cropBorder
        self.bitDepth = bitDepth
        self.numBytes = 2 ** bitDepth - 1
        self.cropSizeHeight = self.targetShapeHeight - self.maxPixelShift
        self.cropSizeWidth = self.targetShapeWidth - self.maxPixelShift
        self.pi = 0.7                                     # SobelL1Mix weight (models/loss.py:21)
        self.eta = 0.25                                   # SSIM share of the l1msssim mixture (models/loss.py:35)

    def _check(self, pred):
        if pred.shape[1] != self.targetShapeHeight or pred.shape[2] != self.targetShapeWidth:
            raise ValueError("Losses(targetShape=%r) got a %dx%d prediction"
                             % ((self.targetShapeHeight, self.targetShapeWidth, self.targetShapeChannels),
                                pred.shape[1], pred.shape[2]))

    def _check_crop(self, limit, what):
        """The LDS-bound losses: refuse a too-large targetShape here, by name, before anything is launched."""
        crop = max(self.cropSizeHeight, self.cropSizeWidth)
        if crop > limit:
            raise ValueError("%s: crop %d (targetShape %d - 2 * cropBorder %d) exceeds the limit of %d pixels of this loss"
                             % (what, crop, max(self.targetShapeHeight, self.targetShapeWidth), self.cropBorder, limit))

    def shiftCompensatedL1Loss(self, patchHR, maskHR, predPatchHR):
        """models/loss.py:73-84 -> scalar: mean over the batch of the minimum masked, bias-corrected L1."""
        hr, m, pred = _prep(patchHR, maskHR, predPatchHR)
        self._check(pred)
        return torch.ops.probav.shift_loss(pred, hr, m, self.cropBorder, self.bitDepth, 1)[0]

    def shiftCompensatedL2Loss(self, patchHR, maskHR, predPatchHR):
        """models/loss.py:55-71."""
        hr, m, pred = _prep(patchHR, maskHR, predPatchHR)
        self._check(pred)
        return torch.ops.probav.shift_loss(pred, hr, m, self.cropBorder, self.bitDepth, 2)[0]

    def shiftCompensatedcPSNR(self, patchHR, maskHR, predPatchHR):
        """models/loss.py:37-53 -> [B]: maximum cPSNR over the shifts (no gradient, as in trainStep)."""
        hr, m, pred = _prep(patchHR, maskHR, predPatchHR)
        self._check(pred)
        with torch.no_grad():
            f, _, _ = torch.ops.probav.shift_metrics(hr, m, pred.detach(), self.cropBorder, self.bitDepth)
        return f[2]

    def evaluate_all(self, patchHR, maskHR, predPatchHR):
        """One launch, everything it computes: dict(l1[B], l2[B], cpsnr[B], arg_l1[B], arg_l2[B], mean_l1, mean_l2)."""
        hr, m, pred = _prep(patchHR, maskHR, predPatchHR)
        self._check(pred)
        with torch.no_grad():
            f, arg, means = torch.ops.probav.shift_metrics(hr, m, pred.detach(), self.cropBorder, self.bitDepth)
        return {"l1": f[0], "l2": f[1], "cpsnr": f[2], "arg_l1": arg[0], "arg_l2": arg[1],
                "mean_l1": means[0], "mean_l2": means[1]}

    def shiftCompensatedL1EdgeLoss(self, patchHR, maskHR, predPatchHR):
        """models/loss.py:86-97 (cfg loss = sobel_l1_mix): pi * L1 + (1 - pi) * Sobel-edge L1, minimum over the shifts, batch mean."""
        hr, m, pred = _prep(patchHR, maskHR, predPatchHR)
        self._check(pred)
        self._check_crop(L1EDGE_MAX_CROP, "shiftCompensatedL1EdgeLoss (sobel_l1_mix)")
        return torch.ops.probav.shift_l1edge_loss(pred, hr, m, self.cropBorder, float(self.pi))[0]

    def shiftCompensatedRevSSIM(self, patchHR, maskHR, predPatchHR):
        """models/loss.py:99-110 (cfg loss = l1msssim): the batch-level multi-scale SSIM / weighted-L1 mixture, minimum over the shifts."""
        hr, m, pred = _prep(patchHR, maskHR, predPatchHR)
        self._check(pred)
        self._check_crop(REVSSIM_MAX_CROP, "shiftCompensatedRevSSIM (l1msssim)")
        return torch.ops.probav.revssim_loss(pred, hr, m, self.cropBorder, self.bitDepth, float(self.eta))[0]
