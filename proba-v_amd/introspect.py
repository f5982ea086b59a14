"""Introspection of a forward pass for parity checks (used by tests/ and __graft_entry__.smoke(); nothing on the product path calls it).

The gradient of the network is discontinuous in its ReLU gates; an fp32 and an fp64 evaluation decide the few gates whose pre-activation
is ~0 differently.  `device_gates` reads the decisions the HIP forward pass actually took, so that a checker can evaluate its own
gradient at the same gates and compare what is left: the arithmetic of the kernels (1e-3 of the per-tensor max norm).
"""
import ctypes

import torch

from . import _lib


def pointwise_pair_is_fused(m):
    """Whether the engine of `m` runs expConv + ReLU + decConv as ONE launch each way now (`probav_engine_pair_kind`, csrc/engine.hip: Family::pw_fused):
    in every family but 0 at the channel counts the tuned kernels take (mfma_pw_supported, csrc/kernels_mfma.hip: 32 -> 256 -> D <= 26; kind 1), or, with
    the general matrix route and its pair switch on, at the counts gemm_pw_supported takes (csrc/kernels_gemm_pw.hip; kind 2).  Otherwise the hidden tensor
    passes through memory and each 1x1x1 layer is a launch of its own."""
    return _lib.lib().probav_engine_pair_kind(m._handle()) != 0


def _effective_weights(m, flat_used, wc):
    """The effective (weight-normalised) filters of every layer as the pass used them, one flat tensor in layer order ([tap][Cin][Cout] each): the first
    block of the weight cache when the pass ran from it, otherwise what probav_wn_forward -- the launch the pass itself starts with -- makes of the parameters."""
    L, h = _lib.lib(), m._handle()
    nw, nc = L.probav_weff_count(h), L.probav_cout_total(h)
    if wc is not None:
        return wc[:nw]
    weff, weffT, invn = (torch.empty(n, device=flat_used.device) for n in (nw, nw, nc))
    _lib.check(L.probav_wn_forward(h, _lib.ptr(flat_used), _lib.ptr(weff), _lib.ptr(weffT), _lib.ptr(invn), _lib.current_stream()), "probav_wn_forward")
    return weff


def _unfused_hidden(m, flat_used, weff, x, B, T, block):
    """relu(expConv_block(x)) [B * voxels * E] of an UN-fused pointwise pair, as the reverse pass recomputes it: backward_impl (csrc/engine.hip) launches that
    1x1x1 layer without operand fragments, which conv_route sends to the generic direct kernel in every family -- the single-operator entry point's impl 0 --
    on the saved block input `x`, the effective weights and the bias.  Its signs are the gates the backward-filter and backward-data launches of expConv
    were handed."""
    L = _lib.lib()
    F, E = m.numFilters, m.numFilters * m.expRate
    hin = m.patchSizeLR + m.maxShift
    off = 0
    for Lh in m.layers:
        if Lh.name == "expConv_%d" % block:
            break
        off += Lh.b_off - Lh.v_off
    assert Lh.name == "expConv_%d" % block and Lh.vshape == (1, 1, 1, F, E)
    w = weff[off: off + F * E]
    bias = flat_used[Lh.b_off: Lh.b_off + E]
    g = (ctypes.c_int32 * 17)(B, hin, hin, T, F, hin, hin, T, E, 1, 1, 1, 0, 0, 0, 0, 1)
    hid = torch.empty(B * hin * hin * T * E, device=x.device)
    _lib.check(L.probav_conv3d_forward(ctypes.byref(g), _lib.ptr(x), None, _lib.ptr(w), _lib.ptr(bias), None, _lib.ptr(hid), 0, _lib.current_stream()),
               "probav_conv3d_forward")
    return hid


def device_gates(m, flat_used, B, T=9, samples=None):
    """{layer: bool array}: the ReLU decisions of the last training forward of `m` (batch B, T frames), read from the saved activations
    (a post-ReLU value is > 0 exactly where the gate is open: `probav_workspace_view`) and, for the hidden tiles of the fused pointwise pair, which
    never reach memory, recomputed by the forward kernel itself (`probav_debug_hidden`; the tuned pair: kernel families 3 and 4 -- the fp32-MFMA families
    do not expose theirs, and the call raises; the general matrix route's pair: every family).  Where the pair runs un-fused (family 0; any family at channel counts other than 32 -> 256 -> D <= 26:
    `pointwise_pair_is_fused`) the hidden tensor is rebuilt from the saved block input with the launch the reverse pass itself recomputes it with
    (`_unfused_hidden`).  Needs the pass's workspace alive: run the forward with PROBAV_KEEP_WS=1, or call this before the backward pass releases it.
    samples (optional): only these samples of the batch, in this order -- the gates of a sub-batch of a large batch (every saved tensor is
    sample-major), sliced on the device.
    The fused hidden tiles come from the 32x32x16 arrangement of the fused forward kernel, which is the one the BACKWARD pass recomputes them
    with: these are the gates the gradient was taken at.  The forward pass proper (pw_fwd_h3k_kernel: 16x16x32) sums the same products in
    another order; a pre-activation that is zero to the last bit can be open in one and closed in the other -- its forward contribution
    is its value, ~0 (csrc/kernels_x6.hip, the comment above that kernel)."""
    L = _lib.lib()
    h, ws = m._handle(), m._workspace(B, True)
    wc = m.weight_cache()                    # the cache the forward pass ran from (None: it recomputed the weights into its workspace)
    hin = m.patchSizeLR + m.maxShift

    def view(kind, idx):
        off, cnt = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(L.probav_workspace_view(h, B, 1, kind, idx, ctypes.byref(off), ctypes.byref(cnt)), "probav_workspace_view")
        return ws[off.value: off.value + cnt.value]
    def pick(t):                                     # [B * per] (or any sample-major flat tensor) -> the chosen samples
        if samples is None:
            return t
        return t.view(B, -1)[torch.as_tensor(list(samples), device=t.device)].reshape(-1)
    gates = {"mainConv1": (pick(view(0, 0)) > 0).cpu().numpy(), "residConv1": (pick(view(3, 0)) > 0).cpu().numpy()}
    nvox = B * hin * hin * T
    # (the un-fused route in x6 arithmetic, `probav_engine_gemm_arith` == 1: its bits are not the direct kernel's, so the hidden tensor is recomputed by the
    # route's own expConv launch, the one the reverse pass runs -- probav_debug_hidden serves that too)
    if pointwise_pair_is_fused(m) or (m.numResBlocks and L.probav_engine_gemm_arith(h) == 1):
        hid = torch.empty(nvox * m.numFilters * m.expRate, device=ws.device)
        dec = torch.empty(nvox * int(m.numFilters * m.decayRate), device=ws.device)      # the launch's regular output (decConv), discarded
        for i in range(m.numResBlocks):
            _lib.check(L.probav_debug_hidden(h, _lib.ptr(flat_used), _lib.ptr(ws), ws.numel() * 4, B, i, _lib.ptr(hid), _lib.ptr(dec), _lib.ptr(wc),
                                             _lib.current_stream()), "probav_debug_hidden")
            gates["expConv_%d" % i] = (pick(hid) > 0).cpu().numpy()
    elif m.numResBlocks:
        weff = _effective_weights(m, flat_used, wc)
        for i in range(m.numResBlocks):
            hid = _unfused_hidden(m, flat_used, weff, view(0, i), B, T, i)
            gates["expConv_%d" % i] = (pick(hid) > 0).cpu().numpy()
    k = 0
    while True:
        try:
            gates["convReducer_%d" % (k + 1)] = (pick(view(2, k)) > 0).cpu().numpy()
        except ValueError:
            break
        k += 1
    return gates


def hidden_tile(m, flat_used, B, block, T=9, from_forward_kernel=False):
    """relu(expConv_block(x)) [B, voxels, 256] of the last training forward of `m`, each sample at its hidden tile's own power-of-two scale, as the
    32x32x16 arrangement evaluates it (default: the order of additions the reverse pass recomputes the tile -- and decides its gates -- in) or as the
    forward kernel itself does (pw_fwd_h3k_kernel; `probav_debug_hidden_from_forward_kernel`)."""
    L = _lib.lib()
    h, ws = m._handle(), m._workspace(B, True)
    wc = m.weight_cache()
    hin = m.patchSizeLR + m.maxShift
    nvox = B * hin * hin * T
    hid = torch.empty(nvox * m.numFilters * m.expRate, device=ws.device)
    dec = torch.empty(nvox * int(m.numFilters * m.decayRate), device=ws.device)
    _lib.check(L.probav_debug_hidden_from_forward_kernel(1 if from_forward_kernel else 0), "probav_debug_hidden_from_forward_kernel")
    try:
        _lib.check(L.probav_debug_hidden(h, _lib.ptr(flat_used), _lib.ptr(ws), ws.numel() * 4, B, block, _lib.ptr(hid), _lib.ptr(dec), _lib.ptr(wc),
                                         _lib.current_stream()), "probav_debug_hidden")
    finally:
        _lib.check(L.probav_debug_hidden_from_forward_kernel(0), "probav_debug_hidden_from_forward_kernel")
    return hid.view(B, -1, m.numFilters * m.expRate)
