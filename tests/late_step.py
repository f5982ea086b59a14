"""One whole training step through autograd on a late stream (tests/late_stream.py): WDSRModel forward, shiftCompensatedL1Loss, backward, for the shipped network at
batch 2.  The input, the target and the flat parameters hold zeros until their values are copied in on the stream, behind its delay; prediction, loss and flat gradient
must be those of the default stream bit for bit, and the step must have been enqueued before the delay has passed.  `main()` is the same for a child process
(PROBAV_NO_SIDE_STREAM is read once per process)."""
import sys

import torch


def run(impl, B=2, T=9):
    """-> (failures, early): what differs from the default stream's step, and whether the step came back while the delay was still running."""
    from probav_amd import synth
    from probav_amd.loss import Losses
    from probav_amd.modelsTF import WDSRConv3D
    from tests import late_stream
    dev = torch.device("cuda:0")
    model = WDSRConv3D("late", "NIR", synth.NIR_MEAN, synth.NIR_STD, 6).build(3, 32, (3, 3, 3), 12, 8, 0.8, T, 16, True)
    model.load_variables(synth.synth_params(seed=31, perturb=True, numImgLR=T))
    model = model.to(dev)
    model.set_impl(impl)
    x, hr, mask = (torch.as_tensor(a).to(dev) for a in synth.synth_batch(B, seed=32, numImgLR=T))
    flat = model.flat.detach().clone()
    losses = Losses(targetShape=(48, 48, 1))
    if hasattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch"):
        torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(False)

    def step(x, hr):
        model.flat.grad = None
        pred = model(x, training=True)
        loss = losses.shiftCompensatedL1Loss(hr, mask, pred)
        loss.backward()
        return pred.detach(), loss.detach(), model.flat.grad

    want = [t.clone() for t in step(x, hr)]
    torch.cuda.synchronize()
    s = late_stream.stream(dev)
    with torch.cuda.stream(s):                             # warm-up on the stream: allocator pools, the autograd nodes' streams
        step(x, hr)
    s.synchronize()
    for factor in (1, late_stream.RETRY_FACTOR):
        xl, hl = torch.zeros_like(x), torch.zeros_like(hr)
        with torch.no_grad():
            model.flat.zero_()
        model.invalidate_weight_cache()
        torch.cuda.synchronize()
        gate = late_stream.begin(dev, factor, "training step, family %d" % impl)
        with torch.cuda.stream(s):
            with torch.no_grad():
                model.flat.copy_(flat)
            xl.copy_(x)
            hl.copy_(hr)
            got = step(xl, hl)
            early = gate.returned()
            failures = [n for n, g, w in zip(("prediction", "loss", "flat gradient"), got, want) if not torch.equal(g, w)]       # (read through the stream alone)
        s.synchronize()
        if early:
            break
    return failures, early


def main():
    failures, early = run(int(sys.argv[1]))
    print("LATE_STEP failures=%s early=%s" % (",".join(failures) or "none", early))
    from tests import late_stream
    print(late_stream.summary())


if __name__ == "__main__":
    main()
