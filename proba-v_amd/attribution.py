"""Frame attribution: which LR frames and pixels a prediction's loss rests on, read off d loss / d x (probav::wdsr_backward_input).

The reference asks for "some ablation study for the important components"; the patches hold their frames from clearest to dirtiest
(utils/dataGenerator.py:326-551), so the share of |d loss / d x| that falls on each frame position says whether the network leans on
the clear frames or on positions -- what `--frame-windows`, `--ensemble-permute` and the frame-order augmentation each assume.

  input_gradient(model, loss_fn, lr, hr, mask, micro_batch) -> dx [N, H, H, T, C] float32 on the model's device
  frame_shares(dx) -> [N, T] float64: frame t's share of sum |dx| of its sample
"""
import torch


def input_gradient(model, loss_fn, lr, hr, mask, micro_batch=128):
    """d loss / d lr of every sample.  lr [N, H, H, T, C], hr / mask [N, S, S, 1] (numpy or torch, any device); loss_fn(hr, mask, pred) is one
    of the `Losses` methods.  The samples run in micro-batches of `micro_batch`; a micro-batch's loss is scaled by its size, so for the
    batch-mean losses (L1, L2, L1-edge) sample i receives the gradient of ITS OWN loss whatever the micro-batch size.  The parameters'
    gradients are computed by the same pass and dropped (there is no dx-only pass); `model.flat.grad` is left as it was."""
    dev = model.flat.device
    if micro_batch < 1:
        raise ValueError("micro_batch must be positive")
    to_dev = lambda a, dt: torch.as_tensor(a).to(device=dev, dtype=dt)
    lr, hr = to_dev(lr, torch.float32), to_dev(hr, torch.float32)
    mask = torch.as_tensor(mask).to(device=dev)
    if not (lr.shape[0] == hr.shape[0] == mask.shape[0]) or lr.shape[0] < 1:
        raise ValueError("lr, hr and mask must hold the same, positive number of samples; got %d, %d, %d" % (lr.shape[0], hr.shape[0], mask.shape[0]))
    out = torch.empty(lr.shape, dtype=torch.float32, device=dev)
    for i in range(0, lr.shape[0], micro_batch):
        x = lr[i:i + micro_batch].detach().clone().requires_grad_(True)
        with torch.enable_grad():
            pred = model(x, training=True)
            loss = loss_fn(hr[i:i + micro_batch], mask[i:i + micro_batch], pred) * float(x.shape[0])
            (dx,) = torch.autograd.grad(loss, [x])
        out[i:i + micro_batch] = dx
    return out


def frame_shares(dx):
    """[N, T] float64: sum over (h, w, c) of |dx[n, :, :, t, :]| divided by the sample's total, so a row sums to 1.  A sample whose gradient is
    zero everywhere (a fully masked target) has no preference: its row is the uniform 1 / T.  A sample holding a NaN or inf gets a NaN row."""
    dx = torch.as_tensor(dx)
    if dx.dim() != 5:
        raise ValueError("dx must be [N, H, H, T, C], got %s" % (tuple(dx.shape),))
    a = dx.detach().to(torch.float64).abs().sum(dim=(1, 2, 4))                     # [N, T]
    tot = a.sum(dim=1, keepdim=True)
    T = a.shape[1]
    shares = torch.where(tot > 0, a / torch.where(tot > 0, tot, torch.ones_like(tot)), torch.full_like(a, 1.0 / T))
    bad = ~torch.isfinite(tot)
    return torch.where(bad, torch.full_like(a, float("nan")), shares)
