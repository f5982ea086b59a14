"""FuseNet without a GPU: the numpy statement against a float64 torch composition and its autograd, its FFT form against its direct form, the
23 / 24 padding, the model's protocol, and the fake-tensor trace of a training step."""
import numpy as np
import pytest
import torch

from probav_amd import fusenet_numpy as fn
from tests import fusenet_helpers as fh


@pytest.mark.parametrize("shape", [(1, 17, 17), (2, 48, 48), (1, 49, 83)], ids=str)
def test_statement_equals_the_float64_torch_composition(shape):
    P = fh.params()
    x, g = fh.image(shape), fh.upstream(shape)
    f = fn.forward(x, *P)
    b = fn.backward(g, x, *P, fwd=f)
    t = fh.torch_compose(x, *P, dtype=torch.float64, g=g)
    for key in ("y", "a", "m"):
        assert fh.maxerr(f[key], t[key]) < 1e-10, key
    np.testing.assert_array_equal(f["out"], x.astype(np.float64) + f["m"])
    for key in ("dK", "dgamma", "dbeta"):
        assert fh.maxerr(b[key], t[key]) < 1e-10, key
    # the bias has no effect: autograd's gradient for it is rounding noise around the statement's exact zeros
    assert not b["dbias"].any() and np.abs(t["dbias"]).max() < 1e-10 * np.abs(t["dbeta"]).max()
    f0 = fn.forward(x, P[0], np.zeros(fn.FILTERS), P[2], P[3])
    assert fh.maxerr(f0["m"], f["m"]) < 1e-10


def test_fft_form_equals_direct_form():
    shape = (1, 96, 96)
    P = fh.params()
    x, g = fh.image(shape), fh.upstream(shape)
    fd, ff = fn.forward(x, *P, method="direct"), fn.forward(x, *P, method="fft")
    assert fh.maxerr(ff["y"], fd["y"]) < 1e-9 and fh.maxerr(ff["m"], fd["m"]) < 1e-9
    bd, bf = fn.backward(g, x, *P, method="direct", fwd=fd), fn.backward(g, x, *P, method="fft", fwd=fd)
    assert fh.maxerr(bf["dK"], bd["dK"]) < 1e-9
    assert fn._method(96, 384, None) == "fft" and fn._method(95, 384, None) == "direct"


@pytest.mark.parametrize("method", ["direct", "fft"])
def test_padding_is_23_before_and_24_after(method):
    """A single 1 at (r, c): y[b,ch,r',s'] - bias = K[r-r'+23, c-s'+23, 0, ch] where that index exists, 0 elsewhere."""
    H = W = 96
    K, bias, gamma, beta = fh.params()
    for (r, c) in [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)]:
        x = np.zeros((1, H, W))
        x[0, r, c] = 1.0
        y = fn.conv(x, K, method)[0]                     # [64, H, W]
        want = np.zeros_like(y)
        for rp in range(max(0, r - 24), min(H, r + 24)):
            for sp in range(max(0, c - 24), min(W, c + 24)):
                i, j = r - rp + 23, c - sp + 23
                if 0 <= i < 48 and 0 <= j < 48:
                    want[:, rp, sp] = K[i, j, 0]
        assert np.abs(y - want).max() < 1e-12, (r, c)
        # the reach is asymmetric: 23 rows up from an output pixel, 24 down
        if r == H // 2:
            assert np.abs(y[:, r - 24, c] - K[47, 23, 0]).max() < 1e-12 and np.abs(y[:, r + 23, c] - K[0, 23, 0]).max() < 1e-12
            assert not y[:, r - 25, c].round(12).any() and not y[:, r + 24, c].round(12).any()


def test_model_names_shapes_order_count_and_init():
    from probav_amd.modelsTF import FuseNetConv2D
    import models.modelsTF as alias
    assert alias.FuseNetConv2D is FuseNetConv2D
    m = FuseNetConv2D("fuse", "NIR").build(seed=0)
    assert m.variable_names == ["conv2d/kernel", "conv2d/bias", "instance_normalization/gamma", "instance_normalization/beta"]
    tv = m.trainable_variables
    assert [tuple(t.shape) for t in tv] == [(48, 48, 1, 64), (64,), (64,), (64,)]
    assert m.flat.numel() == 147648 == sum(t.numel() for t in tv) and len(list(m.parameters())) == 1
    assert list(m.state_dict()) == ["flat"]
    limit = (6.0 / (2304 + 147456)) ** 0.5
    k = tv[0].detach()
    assert float(k.abs().max()) <= limit and float(k.abs().max()) > 0.99 * limit and abs(float(k.mean())) < 0.01 * limit
    assert float(tv[1].detach().abs().max()) == 0.0
    for t in tv[2:]:
        assert float(t.detach().abs().max()) <= 0.05 and float(t.detach().abs().max()) > 0.03
    # seeds
    assert torch.equal(FuseNetConv2D("a", "NIR").build(seed=0).flat, m.flat)
    assert not torch.equal(FuseNetConv2D("a", "NIR").build(seed=1).flat, m.flat)
    # the views alias the flat buffer in order
    assert tv[0].data_ptr() == m.flat.data_ptr() and tv[3].data_ptr() == m.flat.data_ptr() + 4 * (147456 + 128)


def test_model_refuses_non_finite_parameters_by_name_and_cpu_inputs(built_lib):
    from probav_amd.modelsTF import FuseNetConv2D
    m = FuseNetConv2D("fuse", "RED").build(seed=2)
    before = m.flat.detach().clone()
    state = {"conv2d": {"kernel": m.trainable_variables[0].detach().clone(), "bias": torch.zeros(64)},
             "instance_normalization": {"gamma": torch.ones(64), "beta": torch.zeros(64)}}
    state["instance_normalization"]["gamma"][7] = float("nan")
    with pytest.raises(ValueError, match="instance_normalization/gamma"):
        m.load_variables(state)
    assert torch.equal(m.flat.detach(), before)
    bad = before.clone()
    bad[5] = float("inf")
    with pytest.raises(ValueError, match="conv2d/kernel"):
        m.load_state_dict({"flat": bad})
    state["instance_normalization"]["gamma"][7] = 1.0
    m.load_variables(state)
    assert float(m.trainable_variables[2].detach().min()) == 1.0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 48, 48))
    with pytest.raises(NotImplementedError):              # the op itself is registered for the device only
        torch.ops.probav.fusenet_forward(torch.zeros(1, 8, 8), m.flat.detach(), True)


def test_make_optimizer_takes_the_plain_path_for_fusenet():
    from probav_amd.modelsTF import FuseNetConv2D
    from probav_amd.trainClass import make_optimizer
    m = FuseNetConv2D("fuse", "NIR").build(seed=0)
    opt = make_optimizer("nadam", m, 1e-4)
    assert opt.model is None and [p is m.flat for p in opt.param_groups[0]["params"]] == [True]


def test_abi_declares_the_fusenet_entry_points():
    from probav_amd import _lib
    for name in ("probav_fusenet_workspace_bytes", "probav_fusenet_forward", "probav_fusenet_backward"):
        assert name in _lib.SIGNATURES


class _Stop(Exception):
    pass


def test_training_step_traces_on_fake_tensors(built_lib):
    """The registered autograd formula and the fake-tensor rules: the joint graph of a FuseNet training step holds the functional reverse op."""
    pytest.importorskip("torch._dynamo")
    from functorch.compile import min_cut_rematerialization_partition
    from torch._functorch.aot_autograd import aot_module_simplified
    from probav_amd import ops                           # noqa: F401
    seen = {}

    def fw_compiler(gm, example_inputs):
        seen["fw"] = gm.print_readable(print_output=False)

        def run(*args):
            raise _Stop()
        return run

    def partition(joint, inputs, **kw):
        seen["joint"] = joint.print_readable(print_output=False)
        return min_cut_rematerialization_partition(joint, inputs, **kw)

    def backend(gm, example_inputs):
        return aot_module_simplified(gm, example_inputs, fw_compiler=fw_compiler, bw_compiler=lambda g, e: g, partition_fn=partition)

    def step(flat, x, hr, mk):
        out, _, _ = torch.ops.probav.fusenet_forward(x, flat, True)
        return torch.ops.probav.shift_loss(out.reshape(2, 96, 96, 1), hr, mk, 3, 16, 1)[0]

    flat = torch.zeros(147648, requires_grad=True)
    x, hr = torch.zeros(2, 96, 96), torch.zeros(2, 96, 96, 1)
    mk = torch.ones(2, 96, 96, 1, dtype=torch.uint8)
    torch._dynamo.reset()
    with pytest.raises(_Stop):
        torch.compile(step, backend=backend, fullgraph=True)(flat, x, hr, mk)
    torch._dynamo.reset()
    assert "probav.fusenet_forward" in seen["fw"]
    assert "probav.fusenet_backward" in seen["joint"] and "probav.shift_loss_backward" in seen["joint"]
    assert "copy_" not in seen["joint"]
    assert "!" not in str(torch.ops.probav.fusenet_backward.default._schema)


# ---- the two new flags ------------------------------------------------------------------------------------------------------------
import importlib.util  # noqa: E402
import os  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_PATH = os.path.join(ROOT, "cfg", "p16t9c85r12.cfg")


def _load(name):
    spec = importlib.util.spec_from_file_location("probav_cli_fuse_" + name, os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _error(parse, args, capsys):
    with pytest.raises(SystemExit) as e:
        parse(args)
    assert e.value.code == 2
    return capsys.readouterr().err.strip().splitlines()[-1].split("error: ", 1)[1]


def test_fuse_flag_parses_and_is_refused_where_it_does_not_apply(capsys):
    from probav_amd import inference
    test_py, evaluate_py = _load("test"), _load("evaluate")
    assert inference.InferenceOptions().fuse is None
    assert [f for f in inference.InferenceOptions.__dataclass_fields__] == ["ensemble", "tiles", "windows", "weights", "fuse"]
    a = test_py.parser(["--cfg", CFG_PATH, "--fuse"])
    b = evaluate_py.parser(["--cfg", CFG_PATH, "--model", "--fuse"])
    assert a.inference.fuse is True and b.inference.fuse is True and a.inference == b.inference
    assert test_py.parser(["--cfg", CFG_PATH]).inference == inference.InferenceOptions()
    assert evaluate_py.parser(["--cfg", CFG_PATH, "--model"]).inference.fuse is None
    both = test_py.parser(["--cfg", CFG_PATH, "--fuse", "--ensemble", "d8", "--tile-stride", "8"]).inference
    assert both.fuse is True and both.ensemble is not None and both.tiles is not None
    assert _error(test_py.parser, ["--cfg", CFG_PATH, "--fuse", "--method", "baseline"], capsys) == \
        "--fuse predicts with the network: it cannot be combined with --method baseline"
    assert _error(test_py.parser, ["--cfg", CFG_PATH, "--fuse", "--reference-loop"], capsys) == \
        "--reference-loop is the reference's plain loop: it cannot be combined with --fuse"
    assert _error(evaluate_py.parser, ["--cfg", CFG_PATH, "--toCompare", ROOT, "--fuse"], capsys) == \
        "--fuse applies to --model (a folder of PNGs is scored as it is)"


def test_train_py_fusion_flags(capsys):
    train_py = _load("train")
    opt = train_py.parser(["--cfg", CFG_PATH, "--modelType", "fusionNet", "--fusion-input", "some/dir"])
    assert (opt.modelType, opt.fusion_input) == ("fusionNet", "some/dir")
    assert train_py.parser(["--cfg", CFG_PATH]).fusion_input is None
    assert _error(train_py.parser, ["--fusion-input", "some/dir"], capsys) == "--fusion-input needs --modelType fusionNet"
    assert _error(train_py.parser, ["--modelType", "fusionNet"], capsys) == \
        "--modelType fusionNet needs --fusion-input DIR (the PNGs of test.py --totest TRAIN)"


def test_fusion_data_pairs_pngs_with_hr_by_id(tmp_path, monkeypatch):
    """train.py's loader: ids through inference.numbered's table (removed ids skipped), a PNG without a partner named in the error."""
    from probav_amd.pngio import imsave_uint16
    train_py = _load("train")
    d = tmp_path
    (d / "pre" / "trimmedArrayDir").mkdir(parents=True)
    (d / "png").mkdir()
    rng = np.random.default_rng(0)
    hr = rng.integers(0, 2 ** 14, (3, 1, 1, 12, 12)).astype(np.float64)
    mask = rng.random(hr.shape) < 0.2
    np.ma.masked_array(hr, mask=mask).dump(str(d / "pre" / "trimmedArrayDir" / "TRAINimgHR_NIR.npy"))
    (d / "removedTrainSetsNIR.txt").write_text("595\n")
    monkeypatch.chdir(d)                                  # removedTrainSets<BAND>.txt is read from the working directory
    imgs = {i: rng.integers(0, 2 ** 16, (12, 12)).astype(np.uint16) for i in (594, 597)}       # rows 0 and 2 (596 is row 1)
    for i, im in imgs.items():
        imsave_uint16(str(d / "png" / ("imgset%04d.png" % i)), im)
    config = {"preprocessing_out": str(d / "pre")}
    X, y, clear, ids = train_py.fusion_data(config, "NIR", str(d / "png"))
    assert ids == [594, 597] and X.shape == y.shape == clear.shape == (2, 12, 12, 1) and X.dtype == y.dtype == np.float32 and clear.dtype == bool
    np.testing.assert_array_equal(X[1, :, :, 0], imgs[597])
    np.testing.assert_array_equal(y[:, :, :, 0], hr[[0, 2], 0, 0])
    np.testing.assert_array_equal(clear[:, :, :, 0], ~mask[[0, 2], 0, 0])
    imsave_uint16(str(d / "png" / "imgset0598.png"), imgs[594])
    with pytest.raises(SystemExit, match="imgset0598.png .id 598. has no partner"):
        train_py.fusion_data(config, "NIR", str(d / "png"))
