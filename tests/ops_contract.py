"""The argument contract of the torch custom ops (probav_amd/ops.py; INTEGRATION.md, 'Custom ops: what an op accepts') as a table of
cases, and a dry-run harness that runs the undecorated implementation of every op on `meta` tensors: no storage is touched, nothing can
launch, and every entry point of the library the op would have called is recorded by name.

  CASES        one well-formed call per op (a few ops have a second one for an optional operand): how to build its operands in an `Env`,
               the compute entry points it makes (each once), its outputs, the operands it writes.
  rows()       one Row per (case, operand, kind): a change of ONE operand (or scalar) of the well-formed call, and what must happen --
               a refusal by exception type, or the same call as on a fresh contiguous clone.
  dry_run()    the harness; run_row() applies a row under it.

The same table drives tests/test_ops_contract_host.py (meta tensors and fake tensors, no GPU) and tests/test_gpu_ops_contract.py."""
import contextlib
import zlib

import numpy as np
import torch

# the engine the recording stub describes: any sizes do, they only have to be told apart
ENGINE = dict(handle=0x5EED0, nparams=1000, weff=640, cout=48, in_shape=(22, 22, 9, 1), out=48, wc_floats=2048)
SAVED_FLOATS, SCRATCH_FLOATS, INFER_FLOATS = 4096, 1536, 512          # per sample

TORCH_DTYPE = {np.dtype(k): v for k, v in ((np.float32, torch.float32), (np.float64, torch.float64), (np.float16, torch.float16), (np.int32, torch.int32),
                                            (np.int64, torch.int64), (np.uint8, torch.uint8), (np.bool_, torch.bool), (np.uint16, torch.uint16),
                                            (np.int16, torch.int16))}


# ---------------------------------------------------------------------------------------------------------------------------------
# the dry-run harness
# ---------------------------------------------------------------------------------------------------------------------------------
def _set(ref, value):
    ref._obj.value = value


def _q_split(e, B, saved, scratch):
    _set(saved, 4 * SAVED_FLOATS * B), _set(scratch, 4 * SCRATCH_FLOATS * B)
    return 0


def _q_layer_info(e, i, name, g, v, b, shp):
    shp._obj[3] = ENGINE["in_shape"][3]
    return 0


def _q_view(e, B, training, kind, index, off, cnt):
    hin, _, T, C = ENGINE["in_shape"]
    _set(off, 0), _set(cnt, B * hin * hin * T * C if kind == 4 else B * (hin - 2) * (hin - 2) * 9)
    return 0


QUERIES = {                                                # size and layout queries: answered, never recorded
    "probav_abi_version": lambda: 7,
    "probav_last_error": lambda: b"",
    "probav_param_count": lambda e: ENGINE["nparams"],
    "probav_weff_count": lambda e: ENGINE["weff"],
    "probav_cout_total": lambda e: ENGINE["cout"],
    "probav_weight_cache_bytes": lambda e: 4 * ENGINE["wc_floats"],
    "probav_workspace_bytes": lambda e, B, training: 4 * B * (SAVED_FLOATS + SCRATCH_FLOATS if training else INFER_FLOATS),
    "probav_workspace_split": _q_split,
    "probav_layer_info": _q_layer_info,
    "probav_workspace_view": _q_view,
    "probav_revssim_scratch_bytes": lambda B, border: (2 * border + 1) ** 2 * B * 35 * 8,
    "probav_grad_guard_scratch_bytes": lambda n: 128 * 8,
    "probav_ssim_scratch_bytes": lambda N, S, border: 64,
    "probav_conv3d_wgrad_scratch_bytes": lambda g, impl: 256,
    "probav_pw_backward_scratch_bytes": lambda D: 256,
    "probav_fusenet_workspace_bytes": lambda B, H, W, backward: 512,
}


class StubLib:
    """Stands for the loaded library: a query answers from ENGINE, every other entry point records its name and returns PROBAV_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name in QUERIES:
            return QUERIES[name]
        if not name.startswith("probav_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append(name)
            return 0
        return entry


def _require_meta(t, name):
    """`meta` stands for the device, anything else for a foreign one."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor, got %r" % (name, type(t)))
    if t.device.type != "meta":
        raise RuntimeError("%s lives on %s: the WDSR-B hot path runs only as HIP kernels on a gfx950 device (no CPU fallback)" % (name, t.device))
    return t


@contextlib.contextmanager
def dry_run(device_check=_require_meta):
    """Under it the ops of probav_amd.ops.IMPLS can be called with meta tensors: the library, the pointer and stream getters, the memory-pool
    context, the Gaussian-tap upload and the device check are replaced; yields the recording stub."""
    from probav_amd import _lib, ops
    stub = StubLib()
    patches = [(_lib, "lib", lambda: stub), (_lib, "ptr", lambda t: None), (_lib, "current_stream", lambda: None), (_lib, "require_device", device_check),
               (ops, "_ws_pool", lambda *a, **k: None), (torch.cuda, "use_mem_pool", lambda *a, **k: contextlib.nullcontext()),
               (ops, "_gauss11", lambda device: torch.empty(11, dtype=torch.float64, device=device))]
    saved = [(o, n, getattr(o, n)) for o, n, _ in patches]
    sizes = dict(ops._ENGINE_SIZES)
    ops._ENGINE_SIZES.clear()
    try:
        for o, n, v in patches:
            setattr(o, n, v)
        yield stub
    finally:
        for o, n, v in saved:
            setattr(o, n, v)
        ops._ENGINE_SIZES.clear()
        ops._ENGINE_SIZES.update(sizes)


# ---------------------------------------------------------------------------------------------------------------------------------
# where the operands of a case live
# ---------------------------------------------------------------------------------------------------------------------------------
class Env:
    """kind 'meta': meta tensors, the stub's engine.  'fake': tensors made inside a FakeTensorMode ('cuda' the device, 'cpu' the foreign one), the
    stub's engine.  'cuda': real tensors and a real engine (tests/test_gpu_ops_contract.py supplies `engine`)."""

    def __init__(self, kind, engine=None):
        self.kind, self.real = kind, kind == "cuda"
        self.device = torch.device({"meta": "meta", "fake": "cuda", "cuda": "cuda:0"}[kind])
        self.engine = engine if engine is not None else StubEngine(self)

    def put(self, a):
        a = np.asarray(a)
        if self.real:
            return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        return torch.empty(a.shape, dtype=TORCH_DTYPE[a.dtype], device=self.device)

    def empty(self, shape, dtype):
        return torch.empty(tuple(shape), dtype=dtype, device=self.device)

    def foreign(self, t):
        return torch.zeros(tuple(t.shape), dtype=t.dtype, device="cpu")


class StubEngine:
    def __init__(self, env):
        self.env = env
        self.handle, self.nparams, self.out, self.in_shape = ENGINE["handle"], ENGINE["nparams"], ENGINE["out"], ENGINE["in_shape"]
        self.weff, self.cout, self.wc_floats = ENGINE["weff"], ENGINE["cout"], ENGINE["wc_floats"]

    def flat(self):
        return self.env.empty((self.nparams,), torch.float32)

    def x(self, B):
        return self.env.empty((B,) + self.in_shape, torch.float32)

    def wcache(self):
        return self.env.empty((self.wc_floats,), torch.float32)

    def ws(self, B, wcache=False):
        """The saved state of a training pass of batch B (from the weight cache or not)."""
        return self.env.empty((SAVED_FLOATS * B,), torch.float32)

    def inv_norm(self):
        return self.env.empty((self.cout,), torch.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# the well-formed calls
# ---------------------------------------------------------------------------------------------------------------------------------
F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
ANY_SIZE = object()           # Case.size[operand]: nothing for the operand's size to disagree with


class Case:
    """id: the op name, '+x' for a second call of the op with its optional operand x.  build(E, rng) -> [(argument, value)] in schema order.
    entries: the compute entry points, each called once.  outs(args) -> [(shape, dtype)] of the outputs (None: the op returns nothing).
    mutated: operands written in place.  compare: the outputs a device run compares (default all).  size: operand -> the shape that disagrees
    (default: one more along dimension 0).  rank: operands whose rank is fixed (one more leading dimension is refused).  scalars: (argument, bad
    value).  empty: (accepted, {operand: empty shape}, entries then, output shapes then).  no_expand: operands whose values must differ (a
    zero-stride view of them is no well-formed call: set offsets, and the engine's own workspace and weight cache, whose content is the library's)."""

    def __init__(self, id, build, entries, outs, mutated=(), compare=None, size=None, rank=(), scalars=(), empty=None, no_expand=()):
        self.id, self.op = id, id.split("+")[0]
        self.build, self.entries, self.outs, self.mutated, self.compare = build, tuple(entries), outs, tuple(mutated), compare
        self.size, self.rank, self.scalars, self.empty, self.no_expand = dict(size or {}), tuple(rank), tuple(scalars), empty, tuple(no_expand)

    def args(self, E):
        return self.build(E, np.random.default_rng(zlib.crc32(self.id.encode())))


def _f(rng, *shape, scale=1.0):
    return (rng.normal(size=shape) * scale).astype(np.float32)


def _recipe(rng, B, N, T, grouped=False):
    r = np.zeros((B, 3 + T), np.int32)
    r[:, 0] = np.arange(B) * N // B if grouped else rng.integers(0, N, B)
    r[:, 1], r[:, 2] = rng.integers(0, 4, B), rng.integers(0, 4, B)
    r[:, 3:] = np.stack([rng.permutation(T) for _ in range(B)])
    return r


def _loss_inputs(E, rng, B=3, S=12):
    hr = rng.integers(0, 2 ** 14, (B, S, S, 1)).astype(np.float32)
    pred = (hr + rng.normal(0, 200, hr.shape)).astype(np.float32)
    mask = (rng.random((B, S, S, 1)) < 0.8).astype(np.uint8)
    return E.put(pred), E.put(hr), E.put(mask)


LOSS_B, LOSS_S, LOSS_BORDER = 3, 12, 2
NS = (2 * LOSS_BORDER + 1) ** 2
COEF = [("lr", 5e-4), ("beta_1", 0.9), ("beta_2", 0.999), ("eps", 1e-7), ("c_g", 1.0), ("c_m", 0.5), ("c_v", 2.0)]
CTL_ONE = np.array([0x3F800000, 0, 0, 0], np.int32)                   # {scale = 1.0f, skip = 0, skipped_total = 0, norm = 0}


def _b_wdsr_forward(wc):
    def build(E, rng):
        g = E.engine
        return [("flat", g.flat()), ("x", g.x(2)), ("engine", g.handle), ("out_size", g.out), ("training", True), ("wcache", g.wcache() if wc else None)]
    return build


def _b_wdsr_backward(wc):
    def build(E, rng):
        g = E.engine
        return [("flat", g.flat()), ("dy", E.put(_f(rng, 2, g.out, g.out, 1))), ("ws", g.ws(2, wc)), ("engine", g.handle), ("wcache", g.wcache() if wc else None)]
    return build


def _b_shift_metrics(E, rng):
    p, h, m = _loss_inputs(E, rng)
    return [("hr", h), ("mask", m), ("pred", p), ("border", LOSS_BORDER), ("bit_depth", 16)]


def _b_shift_loss(E, rng):
    p, h, m = _loss_inputs(E, rng)
    return [("pred", p), ("hr", h), ("mask", m), ("border", LOSS_BORDER), ("bit_depth", 16), ("which", 1)]


def _arg(E, B):
    return E.put(np.full((B,), NS // 2, np.int32))                   # the centre shift: valid for every sample


def _b_shift_loss_backward(E, rng):
    p, h, m = _loss_inputs(E, rng)
    return [("hr", h), ("mask", m), ("pred", p), ("arg", _arg(E, LOSS_B)), ("upstream", E.put(np.array([1.3], np.float32))), ("border", LOSS_BORDER),
            ("which", 2)]


def _b_l1edge(E, rng):
    p, h, m = _loss_inputs(E, rng)
    return [("pred", p), ("hr", h), ("mask", m), ("border", LOSS_BORDER), ("pi", 0.7)]


def _b_l1edge_backward(E, rng):
    p, h, m = _loss_inputs(E, rng)
    return [("hr", h), ("mask", m), ("pred", p), ("arg", _arg(E, LOSS_B)), ("upstream", E.put(np.array([1.3], np.float32))), ("border", LOSS_BORDER),
            ("pi", 0.7)]


def _b_revssim(E, rng):
    p, h, m = _loss_inputs(E, rng)
    return [("pred", p), ("hr", h), ("mask", m), ("border", LOSS_BORDER), ("bit_depth", 16), ("eta", 0.25)]


def _b_revssim_backward(E, rng):
    p, h, m = _loss_inputs(E, rng)
    if E.real:                                             # the saved state of the matching forward pass
        _, arg, mom = torch.ops.probav.revssim_loss(p, h, m, LOSS_BORDER, 16, 0.25)
    else:
        arg, mom = E.empty((1,), I32), E.empty((NS, LOSS_B, 5, 7), F64)
    return [("hr", h), ("mask", m), ("pred", p), ("arg", arg), ("moments", mom), ("upstream", E.put(np.array([1.3], np.float32))),
            ("border", LOSS_BORDER), ("bit_depth", 16), ("eta", 0.25)]


def _optim_state(E, rng, n, theta=None):
    theta = E.put(_f(rng, n)) if theta is None else theta
    return [("theta", theta), ("grad", E.put(_f(rng, n, scale=0.1))), ("m", E.put(_f(rng, n, scale=0.01))), ("v", E.put(np.abs(_f(rng, n, scale=0.01))))]


def _b_nadam(E, rng):
    return _optim_state(E, rng, 1000) + COEF


def _b_optimizer_wn(E, rng):
    g = E.engine
    return _optim_state(E, rng, g.nparams, g.flat()) + [("wcache", g.wcache()), ("engine", g.handle)] + COEF


def _b_grad_guard(E, rng):
    return [("grad", E.put(_f(rng, 1000))), ("ctl", E.put(np.zeros(4, np.int32))), ("scratch", E.put(np.zeros(128, np.float64))), ("clipnorm", 1.5),
            ("skip_nonfinite", True)]


def _b_nadam_guarded(E, rng):
    return _optim_state(E, rng, 1000) + [("ema", E.put(_f(rng, 1000))), ("ctl", E.put(CTL_ONE))] + COEF + [("ema_momentum", 0.99)]


def _b_optimizer_wn_guarded(E, rng):
    g = E.engine
    return (_optim_state(E, rng, g.nparams, g.flat()) + [("wcache", g.wcache()), ("ema", E.put(_f(rng, g.nparams))), ("ctl", E.put(CTL_ONE)),
                                                          ("engine", g.handle)] + COEF + [("ema_momentum", 0.99)])


def _b_weight_cache_build(E, rng):
    g = E.engine
    return [("theta", g.flat()), ("wcache", g.wcache()), ("engine", g.handle)]


def _b_clip_round(E, rng):
    return [("x", E.put(_f(rng, 5, 6, scale=40000.0))), ("lo", 0.0), ("hi", 65536.0)]


SCORE_N, SCORE_S = 2, 16


def _b_score(E, rng):
    hr = rng.integers(0, 2 ** 14, (SCORE_N, SCORE_S, SCORE_S)).astype(np.uint16)
    sr = np.clip(hr.astype(np.int64) + rng.integers(-300, 300, hr.shape), 0, 65535).astype(np.uint16)
    return [("sr", E.put(sr)), ("hr", E.put(hr)), ("mask", E.put((rng.random(hr.shape) < 0.8).astype(np.uint8))), ("border", 1)]


AUG = dict(N=3, H=6, T=3, C=1, S=12, B=4)


def _b_augment(E, rng):
    a = AUG
    return [("lr", E.put(_f(rng, a["N"], a["H"], a["H"], a["T"], a["C"]))), ("hr", E.put(_f(rng, a["N"], a["S"], a["S"], 1))),
            ("mask", E.put((rng.random((a["N"], a["S"], a["S"], 1)) < 0.8).astype(np.uint8))), ("recipe", E.put(_recipe(rng, a["B"], a["N"], a["T"])))]


def _b_expand(E, rng):
    a = AUG
    return [("lr", E.put(_f(rng, a["N"], a["H"], a["H"], a["T"], a["C"]))), ("recipe", E.put(_recipe(rng, a["B"], a["N"], a["T"])))]


def _b_reduce(E, rng):
    N, V, S, T = 2, 4, 8, 3
    return [("sr", E.put(_f(rng, N * V, S, S, scale=20000.0))), ("recipe", E.put(_recipe(rng, N * V, N, T, grouped=True))), ("V", V), ("lo", 0.0),
            ("hi", 65536.0), ("final_round", True), ("sets", 0), ("grid", 0)]


def _b_tile_blend(E, rng):
    n, S = 2, 8
    return [("sr", E.put(_f(rng, n * n, S, S, scale=20000.0))), ("w", E.put(rng.integers(1, 1025, S).astype(np.int32))), ("n_images", 1), ("n", n),
            ("hr_stride", 5), ("lo", 0.0), ("hi", 65536.0)]


def _b_windows_gather(E, rng):
    N, T_pre, win = 2, 5, 6
    return [("patches", E.put(_f(rng, N, T_pre, win, win))), ("counts", E.put(rng.integers(0, win * win, (N, T_pre)).astype(np.int32))), ("k", 3),
            ("limit", win * win + 1), ("windows", 2), ("step", 1), ("mode", "clear")]


def _b_windows_reduce(E, rng):
    N, W, S = 2, 3, 8
    return [("sr", E.put(_f(rng, N * W, S, S, scale=20000.0))), ("weight", E.put(rng.integers(1, 30, (N, W)).astype(np.int32))), ("lo", 0.0), ("hi", 65536.0)]


def _b_baseline(E, rng):
    F, H, W = 4, 8, 8
    return [("frames", E.put(rng.integers(0, 2 ** 14, (F, H, W)).astype(np.uint16))), ("clear", E.put((rng.random((F, H, W)) < 0.8).astype(np.uint8))),
            ("set_offsets", E.put(np.array([0, 2, 4], np.int64))), ("mode", "esa")]


def _b_window_counts(E, rng):
    return [("masks", E.put((rng.random((2, 12, 12)) < 0.3).astype(np.uint8))), ("pad", 2), ("win", 5), ("stride", 3)]


CROP = dict(S=2, T_pre=5, H=10, P=4, pad=1, win=6, scale=3, k=3, V=5, B=4)


def _b_crop_batch(E, rng):
    c = CROP
    pos = np.stack([rng.integers(0, c["S"], c["V"]), rng.integers(0, c["H"] - c["P"] + 1, c["V"]), rng.integers(0, c["H"] - c["P"] + 1, c["V"])], 1)
    return [("lr", E.put(_f(rng, c["S"], c["T_pre"], c["H"], c["H"]))), ("lr_mask", E.put((rng.random((c["S"], c["T_pre"], c["H"], c["H"])) < 0.2).astype(np.uint8))),
            ("hr", E.put(_f(rng, c["S"], 3 * c["H"], 3 * c["H"]))), ("hr_clear", E.put((rng.random((c["S"], 3 * c["H"], 3 * c["H"])) < 0.8).astype(np.uint8))),
            ("positions", E.put(pos.astype(np.int32))), ("recipe", E.put(_recipe(rng, c["B"], c["V"], c["k"]))), ("P", c["P"]), ("pad", c["pad"]),
            ("win", c["win"]), ("scale", c["scale"]), ("limit", c["win"] ** 2 + 1)]


CONV_X, CONV_W = (1, 6, 5, 4, 25), (3, 3, 3, 25, 32)
CONV_Y = (1, 6, 5, 4, 32)


def _b_conv_fwd(extra):
    def build(E, rng):
        return [("x", E.put(_f(rng, *CONV_X))), ("w", E.put(_f(rng, *CONV_W, scale=0.05))), ("bias", E.put(_f(rng, 32))), ("pad", [1, 1, 1]),
                ("reflect_hw", False), ("relu", False), ("skip", E.put(_f(rng, *CONV_Y)) if extra else None), ("gate", E.put(_f(rng, *CONV_X)) if extra else None),
                ("impl", 4)]
    return build


def _b_conv_wgrad(extra):
    def build(E, rng):
        return [("x", E.put(_f(rng, *CONV_X))), ("dy", E.put(_f(rng, *CONV_Y))), ("ksize", [3, 3, 3]), ("pad", [1, 1, 1]), ("reflect_hw", False),
                ("gate", E.put(_f(rng, *CONV_Y)) if extra else None), ("impl", 4)]
    return build


PW_VOX, PW_D = 40, 25


def _pw_weights(E, rng):
    return [("w1", E.put(_f(rng, 32, 256, scale=1 / 6))), ("b1", E.put(_f(rng, 256, scale=0.1))), ("w2", E.put(_f(rng, 256, PW_D, scale=1 / 16)))]


def _b_pw_fwd(E, rng):
    return [("x", E.put(_f(rng, PW_VOX, 32)))] + _pw_weights(E, rng) + [("b2", E.put(_f(rng, PW_D, scale=0.1))), ("vox_per_sample", 0), ("impl", 4)]


def _b_pw_bwd(E, rng):
    return ([("x", E.put(_f(rng, PW_VOX, 32))), ("d_dec", E.put(_f(rng, PW_VOX, PW_D))), ("d_skip", E.put(_f(rng, PW_VOX, 32)))] + _pw_weights(E, rng)
            + [("vox_per_sample", 0), ("impl", 4)])


def _b_wn_fwd(E, rng):
    return [("flat", E.engine.flat()), ("engine", E.engine.handle)]


def _b_wn_bwd(E, rng):
    g = E.engine
    return [("flat", g.flat()), ("dweff", E.put(_f(rng, g.weff))), ("inv_norm", g.inv_norm()), ("engine", g.handle)]


FUSE_SHAPE, FUSE_PARAMS = (2, 17, 17), 48 * 48 * 64 + 3 * 64


def _fuse_inputs(E, rng):
    x = np.clip(np.rint(6000.0 + rng.normal(0.0, 600.0, FUSE_SHAPE)), 0, 16383).astype(np.float32)
    flat = np.concatenate([_f(rng, 48 * 48 * 64, scale=0.02), _f(rng, 64, scale=0.5), 1.0 + _f(rng, 64, scale=0.1), _f(rng, 64, scale=0.1)])
    return E.put(x), E.put(flat)


def _b_fusenet_fwd(E, rng):
    x, flat = _fuse_inputs(E, rng)
    return [("x", x), ("flat", flat), ("residual", True)]


def _b_fusenet_bwd(E, rng):
    x, flat = _fuse_inputs(E, rng)
    B, H, W = FUSE_SHAPE
    if E.real:
        _, y, stats = torch.ops.probav.fusenet_forward(x, flat, True)
    else:
        y, stats = E.empty((B, H, W, 64), F32), E.empty((B, 64, 2), F32)
    return [("g", E.put(_f(rng, B, H, W, scale=1.0 / (B * H * W)))), ("x", x), ("y", y), ("stats", stats), ("flat", flat)]


def _loss_outs(a):
    return [((), F32), ((LOSS_B,), I32), ((LOSS_B,), F32)]


def _like(name):
    return lambda a: [(tuple(a[name].shape), a[name].dtype)]


_LOSS_EMPTY = {"pred": (0, LOSS_S, LOSS_S, 1), "hr": (0, LOSS_S, LOSS_S, 1), "mask": (0, LOSS_S, LOSS_S, 1)}
_LOSS_SCALARS = (("border", -1), ("border", LOSS_S // 2))
_SCORE_EMPTY = {"sr": (0, SCORE_S, SCORE_S), "hr": (0, SCORE_S, SCORE_S), "mask": (0, SCORE_S, SCORE_S)}
_OPT_EMPTY = {"theta": (0,), "grad": (0,), "m": (0,), "v": (0,)}
_a = AUG
_c = CROP
_ENG = ENGINE

CASES = [
    Case("wdsr_forward", _b_wdsr_forward(False), ["probav_forward"], lambda a: [((2, a["out_size"], a["out_size"], 1), F32), (None, F32)], compare=(0,),
         size={"x": lambda s: s[:1] + (s[1] + 1,) + s[2:]}, rank=("x",), scalars=(("out_size", 0),), empty=(False, {"x": (0,) + _ENG["in_shape"]}, (), None)),
    Case("wdsr_forward+wcache", _b_wdsr_forward(True), ["probav_forward_wc"], lambda a: [((2, a["out_size"], a["out_size"], 1), F32), (None, F32)], compare=(0,),
         size={"x": lambda s: s[:1] + (s[1] + 1,) + s[2:], "wcache": lambda s: (s[0] - 1,)}, empty=(False, {"x": (0,) + _ENG["in_shape"]}, (), None), no_expand=("ws", "wcache")),
    Case("wdsr_backward", _b_wdsr_backward(False), ["probav_backward_split"], _like("flat"), rank=("dy",),
         size={"dy": lambda s: s[:1] + (s[1] + 1,) + s[2:]}, empty=(False, {"dy": (0, _ENG["out"], _ENG["out"], 1), "ws": (0,)}, (), None), no_expand=("ws", "wcache")),
    Case("wdsr_backward+wcache", _b_wdsr_backward(True), ["probav_backward_split"], _like("flat"),
         size={"dy": lambda s: s[:1] + (s[1] + 1,) + s[2:], "wcache": lambda s: (s[0] - 1,)}, empty=(False, {"dy": (0, _ENG["out"], _ENG["out"], 1), "ws": (0,)}, (), None), no_expand=("ws", "wcache")),
    Case("wdsr_backward_input", _b_wdsr_backward(False), ["probav_backward_input"],
         lambda a: [(tuple(a["flat"].shape), F32), ((2,) + tuple(a["_in_shape"]), F32)], rank=("dy",),
         size={"dy": lambda s: s[:1] + (s[1] + 1,) + s[2:]}, empty=(False, {"dy": (0, _ENG["out"], _ENG["out"], 1), "ws": (0,)}, (), None), no_expand=("ws", "wcache")),
    Case("wdsr_backward_input+wcache", _b_wdsr_backward(True), ["probav_backward_input"],
         lambda a: [(tuple(a["flat"].shape), F32), ((2,) + tuple(a["_in_shape"]), F32)],
         size={"dy": lambda s: s[:1] + (s[1] + 1,) + s[2:], "wcache": lambda s: (s[0] - 1,)}, empty=(False, {"dy": (0, _ENG["out"], _ENG["out"], 1), "ws": (0,)}, (), None), no_expand=("ws", "wcache")),
    Case("shift_metrics", _b_shift_metrics, ["probav_shift_loss_forward"], lambda a: [((3, LOSS_B), F32), ((2, LOSS_B), I32), ((2,), F32)], rank=("pred", "hr", "mask"),
         scalars=_LOSS_SCALARS, empty=(False, _LOSS_EMPTY, (), None)),
    Case("shift_loss_backward", _b_shift_loss_backward, ["probav_shift_loss_backward"], _like("pred"), rank=("pred", "hr", "mask"),
         scalars=_LOSS_SCALARS + (("which", 0), ("which", 3)), empty=(False, dict(_LOSS_EMPTY, arg=(0,)), (), None)),
    Case("shift_loss", _b_shift_loss, ["probav_shift_loss_forward"], _loss_outs, rank=("pred", "hr", "mask"),
         scalars=_LOSS_SCALARS + (("which", 0), ("which", 3)), empty=(False, _LOSS_EMPTY, (), None)),
    Case("shift_l1edge_loss", _b_l1edge, ["probav_shift_l1edge_forward"], _loss_outs, rank=("pred", "hr", "mask"), scalars=_LOSS_SCALARS,
         empty=(False, _LOSS_EMPTY, (), None)),
    Case("shift_l1edge_loss_backward", _b_l1edge_backward, ["probav_shift_l1edge_backward"], _like("pred"), rank=("pred", "hr", "mask"), scalars=_LOSS_SCALARS,
         empty=(False, dict(_LOSS_EMPTY, arg=(0,)), (), None)),
    Case("revssim_loss", _b_revssim, ["probav_revssim_forward"], lambda a: [((), F32), ((1,), I32), ((NS, LOSS_B, 5, 7), F64)], rank=("pred", "hr", "mask"),
         scalars=_LOSS_SCALARS, empty=(False, _LOSS_EMPTY, (), None)),
    Case("revssim_loss_backward", _b_revssim_backward, ["probav_revssim_backward"], _like("pred"), rank=("pred", "hr", "mask"), scalars=_LOSS_SCALARS,
         size={"moments": lambda s: s[:1] + (s[1] + 1,) + s[2:]}, empty=(False, dict(_LOSS_EMPTY, moments=(NS, 0, 5, 7)), (), None)),
    Case("nadam_step", _b_nadam, ["probav_nadam_step"], None, mutated=("theta", "m", "v"), empty=(True, _OPT_EMPTY, (), None)),
    Case("optimizer_wn_step", _b_optimizer_wn, ["probav_optimizer_step_fused"], None, mutated=("theta", "m", "v", "wcache"),
         size={"wcache": lambda s: (s[0] - 1,)}, empty=(False, _OPT_EMPTY, (), None)),
    Case("grad_guard", _b_grad_guard, ["probav_grad_guard"], None, mutated=("ctl", "scratch"), size={"scratch": lambda s: (s[0] - 1,), "grad": lambda s: (0,)},
         empty=(False, {"grad": (0,)}, (), None)),
    Case("nadam_step_guarded", _b_nadam_guarded, ["probav_nadam_step_guarded"], None, mutated=("theta", "m", "v", "ema", "ctl"),
         empty=(True, dict(_OPT_EMPTY, ema=(0,)), (), None)),
    Case("optimizer_wn_step_guarded", _b_optimizer_wn_guarded, ["probav_optimizer_step_fused_guarded"], None, mutated=("theta", "m", "v", "wcache", "ema", "ctl"),
         size={"wcache": lambda s: (s[0] - 1,)}, empty=(False, dict(_OPT_EMPTY, ema=(0,)), (), None)),
    Case("weight_cache_build", _b_weight_cache_build, ["probav_weight_cache_build"], None, mutated=("wcache",), size={"wcache": lambda s: (s[0] - 1,)},
         empty=(False, {"theta": (0,)}, (), None)),
    Case("clip_round", _b_clip_round, ["probav_clip_round"], _like("x"), size={"x": ANY_SIZE}, scalars=(("lo", 2.0 ** 17), ("lo", float("nan")), ("hi", float("nan")))),
    Case("esa_shift_moments", _b_score, ["probav_score_moments"], lambda a: [((SCORE_N, 9, 3), I64)], rank=("sr", "hr", "mask"), scalars=(("border", -1), ("border", 4)),
         empty=(True, _SCORE_EMPTY, (), [((0, 9, 3), I64)])),
    Case("esa_shift_cpsnr", _b_score, ["probav_score_moments", "probav_score_select"],
         lambda a: [((SCORE_N,), F64), ((SCORE_N, 2), I32), ((SCORE_N,), F64), ((SCORE_N,), I64)], rank=("sr", "hr", "mask"), scalars=(("border", -1), ("border", 4)),
         empty=(True, _SCORE_EMPTY, (), [((0,), F64), ((0, 2), I32), ((0,), F64), ((0,), I64)])),
    Case("esa_shift_ssim_table", _b_score, ["probav_score_moments", "probav_ssim_table"], lambda a: [((SCORE_N, 9), F64)], rank=("sr", "hr", "mask"),
         scalars=(("border", -1), ("border", 3)), empty=(True, _SCORE_EMPTY, (), [((0, 9), F64)])),
    Case("esa_shift_cssim", _b_score, ["probav_score_moments", "probav_ssim_table", "probav_ssim_select"], lambda a: [((SCORE_N,), F64), ((SCORE_N, 2), I32)],
         rank=("sr", "hr", "mask"), scalars=(("border", -1), ("border", 3)), empty=(True, _SCORE_EMPTY, (), [((0,), F64), ((0, 2), I32)])),
    Case("augment_batch", _b_augment, ["probav_augment_batch"],
         lambda a: [((_a["B"], _a["H"], _a["H"], _a["T"], _a["C"]), F32), ((_a["B"], _a["S"], _a["S"], 1), F32), ((_a["B"], _a["S"], _a["S"], 1), torch.uint8)],
         size={"lr": lambda s: s[:3] + (s[3] + 1,) + s[4:], "recipe": lambda s: (s[0], s[1] + 1)}, rank=("lr", "hr", "mask", "recipe"),
         empty=(True, {"recipe": (0, 3 + _a["T"])}, (), [((0, _a["H"], _a["H"], _a["T"], _a["C"]), F32), ((0, _a["S"], _a["S"], 1), F32), ((0, _a["S"], _a["S"], 1), torch.uint8)])),
    Case("ensemble_expand", _b_expand, ["probav_ensemble_expand"], lambda a: [((_a["B"], _a["H"], _a["H"], _a["T"], _a["C"]), F32)],
         size={"lr": lambda s: s[:3] + (s[3] + 1,) + s[4:], "recipe": lambda s: (s[0], s[1] + 1)}, rank=("lr", "recipe"),
         empty=(True, {"recipe": (0, 3 + _a["T"])}, (), [((0, _a["H"], _a["H"], _a["T"], _a["C"]), F32)])),
    Case("ensemble_reduce", _b_reduce, ["probav_ensemble_reduce"], lambda a: [((2, 8, 8), F32)], rank=("recipe",),
         scalars=(("V", 0), ("V", 257), ("V", 3), ("lo", float("nan")), ("grid", 1)), empty=(False, {"sr": (0, 8, 8), "recipe": (0, 6)}, (), None)),
    Case("tile_blend", _b_tile_blend, ["probav_tile_blend"], lambda a: [((1, 13, 13), F32)], rank=("w",),
         scalars=(("n", 3), ("hr_stride", 0), ("hr_stride", 9), ("lo", 2.0 ** 17), ("hi", float("nan"))), empty=(False, {"sr": (0, 8, 8)}, (), None)),
    Case("frame_windows_gather", _b_windows_gather, ["probav_frame_windows_gather"], lambda a: [((2, 2, 6, 6, 3, 1), F32), ((2, 2), I32), ((2, 2, 3), I32)],
         rank=("patches", "counts"), scalars=(("k", 0), ("windows", 4), ("step", 0), ("limit", -1), ("mode", "median")),
         empty=(False, {"patches": (0, 5, 6, 6), "counts": (0, 5)}, (), None)),
    Case("frame_windows_reduce", _b_windows_reduce, ["probav_frame_windows_reduce"], lambda a: [((2, 8, 8), F32)], rank=("weight",),
         scalars=(("lo", 2.0 ** 17), ("hi", float("nan"))), empty=(False, {"sr": (0, 8, 8), "weight": (0, 3)}, (), None)),
    Case("baseline_upscale_mean", _b_baseline, ["probav_baseline_upscale_mean"], lambda a: [((2, 24, 24), F32), ((2,), I32)], rank=("frames", "clear", "set_offsets"),
         size={"set_offsets": lambda s: (1,)}, scalars=(("mode", "mean"),), empty=(False, {"frames": (0, 8, 8), "clear": (0, 8, 8)}, (), None),
         no_expand=("set_offsets",)),
    Case("window_counts", _b_window_counts, ["probav_window_counts"], lambda a: [((2, 4, 4), I32)], rank=("masks",), size={"masks": lambda s: s[:2] + (40000,)},
         scalars=(("pad", -1), ("pad", 12), ("win", 0), ("win", 17), ("stride", 0)), empty=(False, {"masks": (0, 12, 12)}, (), None)),
    Case("crop_batch", _b_crop_batch, ["probav_crop_batch"],
         lambda a: [((_c["B"], 6, 6, 3, 1), F32), ((_c["B"], 12, 12, 1), F32), ((_c["B"], 12, 12, 1), torch.uint8), ((_c["B"], 3), I32)],
         size={"positions": lambda s: (s[0], 4), "recipe": lambda s: (s[0], 3 + 65)}, rank=("lr", "lr_mask", "hr", "hr_clear", "positions", "recipe"),
         scalars=(("P", 0), ("pad", -1), ("win", 3), ("scale", 0), ("limit", -1)),
         empty=(True, {"recipe": (0, 6)}, (), [((0, 6, 6, 3, 1), F32), ((0, 12, 12, 1), F32), ((0, 12, 12, 1), torch.uint8), ((0, 3), I32)])),
    Case("conv3d_k3_fwd", _b_conv_fwd(False), ["probav_conv3d_forward"], lambda a: [(CONV_Y, F32)], rank=("x", "w", "bias"),
         size={"x": lambda s: s[:4] + (s[4] + 1,), "w": lambda s: s[:3] + (s[3] + 1, s[4])},
         scalars=(("pad", [1, 1]), ("pad", [1, 1, 3]), ("pad", [-1, 1, 1]), ("impl", 5), ("impl", -1)), empty=(False, {"x": (0,) + CONV_X[1:]}, (), None)),
    Case("conv3d_k3_fwd+skip+gate", _b_conv_fwd(True), ["probav_conv3d_forward"], lambda a: [(CONV_Y, F32)], rank=("skip", "gate"),
         size={"x": lambda s: s[:4] + (s[4] + 1,), "w": lambda s: s[:3] + (s[3] + 1, s[4]), "skip": lambda s: s[:4] + (s[4] + 1,), "gate": lambda s: s[:4] + (s[4] + 1,)},
         empty=(False, {"x": (0,) + CONV_X[1:], "gate": (0,) + CONV_X[1:], "skip": (0,) + CONV_Y[1:]}, (), None)),
    Case("conv3d_k3_bwd_weight", _b_conv_wgrad(False), ["probav_conv3d_wgrad"], lambda a: [((3, 3, 3, 25, 32), F32), ((32,), F32)], rank=("x", "dy"),
         scalars=(("ksize", [3, 3]), ("ksize", [3, 0, 3]), ("pad", [1, 1]), ("pad", [1, 1, 3]), ("impl", 5)),
         empty=(False, {"x": (0,) + CONV_X[1:], "dy": (0,) + CONV_Y[1:]}, (), None)),
    Case("conv3d_k3_bwd_weight+gate", _b_conv_wgrad(True), ["probav_conv3d_wgrad"], lambda a: [((3, 3, 3, 25, 32), F32), ((32,), F32)], rank=("gate",),
         size={"gate": lambda s: s[:4] + (s[4] + 1,)}, empty=(False, {"x": (0,) + CONV_X[1:], "dy": (0,) + CONV_Y[1:], "gate": (0,) + CONV_Y[1:]}, (), None)),
    Case("pw_expand_relu_decay_fwd", _b_pw_fwd, ["probav_pw_forward"], lambda a: [((PW_VOX, PW_D), F32)], rank=("w1", "b1", "w2", "b2"),
         size={"x": lambda s: (s[0], s[1] + 1), "w2": lambda s: (s[0], 27)}, scalars=(("vox_per_sample", -1), ("vox_per_sample", 7), ("impl", 5)),
         empty=(False, {"x": (0, 32)}, (), None)),
    Case("pw_expand_relu_decay_bwd", _b_pw_bwd, ["probav_pw_backward"], lambda a: [((PW_VOX, 32), F32), ((32, 256), F32), ((256,), F32), ((256, PW_D), F32), ((PW_D,), F32)],
         rank=("w1", "b1", "w2"), size={"x": lambda s: (s[0], s[1] + 1), "w2": lambda s: (s[0] + 1, s[1])}, scalars=(("vox_per_sample", -1), ("impl", 5)),
         empty=(False, {"x": (0, 32), "d_dec": (0, PW_D), "d_skip": (0, 32)}, (), None)),
    Case("wn_weight_fwd", _b_wn_fwd, ["probav_wn_forward"], lambda a: [((a["_weff"],), F32), ((a["_weff"],), F32), ((a["_cout"],), F32)],
         empty=(False, {"flat": (0,)}, (), None)),
    Case("wn_weight_bwd", _b_wn_bwd, ["probav_wn_backward"], _like("flat"), empty=(False, {"flat": (0,)}, (), None)),
    Case("fusenet_forward", _b_fusenet_fwd, ["probav_fusenet_forward"], lambda a: [(FUSE_SHAPE, F32), (FUSE_SHAPE + (64,), F32), ((FUSE_SHAPE[0], 64, 2), F32)], rank=("x",),
         size={"x": lambda s: (0,) + s[1:]},
         empty=(False, {"x": (0,) + FUSE_SHAPE[1:]}, (), None)),
    Case("fusenet_backward", _b_fusenet_bwd, ["probav_fusenet_backward"], _like("flat"), rank=("x",),
         empty=(False, {"x": (0,) + FUSE_SHAPE[1:], "g": (0,) + FUSE_SHAPE[1:], "y": (0,) + FUSE_SHAPE[1:] + (64,), "stats": (0, 64, 2)}, (), None)),
]
CASE = {c.id: c for c in CASES}


# ---------------------------------------------------------------------------------------------------------------------------------
# the rows: one change of one operand
# ---------------------------------------------------------------------------------------------------------------------------------
def strided(E, t):
    """The same values as a slice of a larger allocation: every second element of the last dimension."""
    big = E.empty(tuple(t.shape[:-1]) + (2 * t.shape[-1],), t.dtype)
    v = big[..., ::2]
    v.copy_(t)
    return v


def _long_dims(t):
    return [d for d, n in enumerate(t.shape) if n > 1]


def permuted(E, t):
    """The same values, dense, with the strides of the first two dimensions longer than 1 exchanged."""
    i, j = _long_dims(t)[:2]
    v = E.empty(tuple(t.transpose(i, j).shape), t.dtype).transpose(i, j)
    v.copy_(t)
    return v


def expanded(E, t):
    """Zero stride: the first slice along the first dimension longer than 1, repeated (the values of the call change; it compares with its own clone)."""
    for d, n in enumerate(t.shape):
        if n > 1:
            return t.narrow(d, 0, 1).expand(t.shape)
    return t.reshape(()).expand(t.shape)


def offset(E, t):
    """The same values as a contiguous view that starts one element into its allocation: off a 16-byte boundary."""
    buf = E.empty((t.numel() + 8,), t.dtype)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def as_bool(E, t):
    return t != 0 if E.real else E.empty(t.shape, torch.bool)


def _cast(dtype):
    def f(E, t):
        return t.to(dtype) if E.real else E.empty(t.shape, dtype)
    return f


def _reshaped(fn):
    def f(E, t):
        return E.empty(fn(tuple(t.shape)), t.dtype)
    return f


WRONG_DTYPES = {torch.float32: (torch.float64, torch.float16), torch.int32: (torch.int64,), torch.uint8: (torch.float32,), torch.bool: (torch.float32,),
                torch.uint16: (torch.int32,), torch.int16: (torch.int32,), torch.float64: (torch.float32,), torch.int64: (torch.int32,)}
LAYOUTS = (("strided", strided), ("permuted", permuted), ("expanded", expanded), ("offset", offset))


class Row:
    """accept: True -> the call goes through as on a contiguous clone; False -> `exc` is raised, naming the op and `operand`, nothing reaches the library."""

    def __init__(self, case, operand, kind, accept, exc, change, entries=None, outs=None):
        self.case, self.operand, self.kind, self.accept, self.exc, self.change = case, operand, kind, accept, exc, change
        self.entries = case.entries if entries is None else tuple(entries)
        self.outs = outs
        self.id = "%s-%s-%s" % (case.id, operand, kind)

    def apply(self, E, args):
        """args: the well-formed [(name, value)] -> the row's."""
        return self.change(E, args)


def _one(name, fn):
    return lambda E, args: [(n, fn(E, v) if n == name else v) for n, v in args]


def _scalar(name, value):
    return lambda E, args: [(n, value if n == name else v) for n, v in args]


def _emptied(shapes):
    return lambda E, args: [(n, E.empty(shapes[n], v.dtype) if n in shapes else v) for n, v in args]


def _rows_of(case):
    E = Env("meta")
    rows = []
    for name, v in case.args(E):
        if not isinstance(v, torch.Tensor):
            continue
        mutated = name in case.mutated
        rows.append(Row(case, name, "device", False, RuntimeError, _one(name, lambda E, t: E.foreign(t))))
        for dt in WRONG_DTYPES[v.dtype]:
            rows.append(Row(case, name, "dtype-%s" % str(dt).split(".")[1], False, ValueError, _one(name, _cast(dt))))
        if name in case.rank:
            rows.append(Row(case, name, "rank", False, ValueError, _one(name, _reshaped(lambda s: (1,) + s))))
        if case.size.get(name) is ANY_SIZE:                # no sibling and no engine to disagree with: the size row is the empty tensor, accepted
            rows.append(Row(case, name, "size", True, None, _one(name, _reshaped(lambda s: (0,) + s[1:])), (), [((0,) + tuple(v.shape[1:]), v.dtype)]))
        else:
            rows.append(Row(case, name, "size", False, ValueError, _one(name, _reshaped(case.size.get(name, lambda s: (s[0] + 1,) + s[1:])))))
        if mutated:
            rows.append(Row(case, name, "noncontiguous", False, ValueError, _one(name, strided)))
            rows.append(Row(case, name, "offset", False, ValueError, _one(name, offset)))
            continue
        for kind, fn in LAYOUTS:
            if kind == "permuted" and len(_long_dims(v)) < 2:
                continue
            if kind == "expanded" and name in case.no_expand:
                continue
            rows.append(Row(case, name, kind, True, None, _one(name, fn)))
        if v.dtype == torch.uint8:
            rows.append(Row(case, name, "bool", True, None, _one(name, as_bool)))
    for name, value in case.scalars:
        rows.append(Row(case, name, "scalar-%r" % (value,), False, ValueError, _scalar(name, value)))
    if case.empty is not None:
        accept, shapes, entries, outs = case.empty
        rows.append(Row(case, next(iter(shapes)), "empty", accept, None if accept else ValueError, _emptied(shapes), entries if accept else None, outs))
    return rows


_ROWS = None


def rows():
    global _ROWS
    if _ROWS is None:
        _ROWS = [r for c in CASES for r in _rows_of(c)]
    return _ROWS


def refusal_rows():
    return [r for r in rows() if not r.accept]


def accepted_rows():
    return [r for r in rows() if r.accept]


# ---------------------------------------------------------------------------------------------------------------------------------
# running a row without a device
# ---------------------------------------------------------------------------------------------------------------------------------
def values(args):
    return [v for _, v in args]


def expected_outs(case, args, E):
    """[(shape, dtype)] of the well-formed call's outputs (shape None: sized by the engine's workspace, not stated)."""
    if case.outs is None:
        return None
    d = dict(args)
    d.update(_in_shape=E.engine.in_shape, _weff=E.engine.weff, _cout=E.engine.cout)
    return case.outs(d)


def contiguous_strides(shape):
    s, out = 1, []
    for n in reversed(shape):
        out.append(s)
        s *= max(int(n), 1)
    return tuple(reversed(out))


def check_outputs(result, want, bool_mask=False):
    """The outputs have the stated shapes and dtypes and standard contiguous strides (bool_mask: a mask output has its operand's dtype)."""
    if want is None:
        assert result is None, result
        return
    result = (result,) if isinstance(result, torch.Tensor) else tuple(result)
    assert len(result) == len(want), (len(result), len(want))
    for i, (t, (shape, dtype)) in enumerate(zip(result, want)):
        assert t.dtype == (torch.bool if bool_mask and dtype == torch.uint8 else dtype), (i, t.dtype, dtype)
        if shape is not None:
            assert tuple(t.shape) == tuple(shape), (i, tuple(t.shape), shape)
        assert t.is_contiguous() and (t.numel() == 0 or all(st == w for n, st, w in zip(t.shape, t.stride(), contiguous_strides(t.shape)) if n > 1)), \
            (i, tuple(t.shape), t.stride())


def bool_output(row):
    """The two ops that hand a mask on give it back in the dtype it came in."""
    return row.kind == "bool" and (row.case.op, row.operand) in (("augment_batch", "mask"), ("crop_batch", "hr_clear"))


def host_check(row):
    """The row on meta tensors under the dry-run harness -> (exception or None, recorded entry points, result)."""
    from probav_amd import ops
    E = Env("meta")
    with dry_run() as stub:
        args = row.apply(E, row.case.args(E))
        try:
            result = ops.IMPLS[row.case.op](*values(args))
        except Exception as e:                             # noqa: BLE001  (the caller judges the type)
            return e, list(stub.calls), None
        return None, list(stub.calls), result


