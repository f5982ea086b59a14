"""The one dispatch of test.py and evaluate.py --model (probav_amd/inference.py::predict) on the device: for every combination of the options
it returns, array for array, what the public testClass call of that combination returns.  Every comparison is an equality."""
import numpy as np
import pytest

from probav_amd import testClass, tiles
from probav_amd.ensemble import EnsembleSpec
from probav_amd.frame_windows import FrameWindowSpec
from probav_amd.inference import InferenceOptions, predict
from probav_amd.tiles import TileSpec

from tests.frame_windows_helpers import WCONFIG
from tests.tiles_helpers import cloudy_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(dev):
    from probav_amd.modelsTF import WDSRConv3D
    return WDSRConv3D("superResolutionNet", "NIR", 8075.2045, 3160.7272, 6).build(3, 32, (3, 3, 3), 12, 8, 0.8, 9, 16, True, seed=0).to(dev)


@pytest.fixture(scope="module")
def frames():
    return cloudy_frames(images=2, T=13, H=128)                        # T_pre = 13 registered frames per set, k = 9 of them per patch


@pytest.fixture(scope="module")
def patches(frames, dev):
    """[2, 64, 22, 22, 9, 1]: the disjoint patches of the frames, what resolverDir holds (tiles.build_tiles at stride P)."""
    return tiles.build_tiles(frames, TileSpec(16), WCONFIG, dev).cpu().numpy()


def _same(got, want, images, side=384):
    assert len(got) == len(want) == images
    for g, w in zip(got, want):
        assert g.shape == w.shape == (side, side, 1) and g.dtype == w.dtype == np.float64
        assert np.array_equal(g, w)


def test_plain(model, patches):
    _same(predict(model, patches, InferenceOptions(), WCONFIG), testClass.evaluate_device(model, patches), 2)
    want = testClass.evaluate_device(model, patches, micro_batch=16, launch_batch=16)
    _same(predict(model, patches, InferenceOptions(), WCONFIG, micro_batch=16, launch_batch=16), want, 2)


def test_self_ensemble(model, patches):
    ens = EnsembleSpec("d8")
    _same(predict(model, patches, InferenceOptions(ensemble=ens), WCONFIG), testClass.evaluate_device(model, patches, ensemble=ens, final="round"), 2)


def test_tiles(model, frames):
    spec, ens = TileSpec(8), EnsembleSpec("d8")
    _same(predict(model, frames, InferenceOptions(tiles=spec), WCONFIG), testClass.evaluate_tiled_frames(model, frames, spec, WCONFIG), 2)
    _same(predict(model, frames, InferenceOptions(ensemble=ens, tiles=spec), WCONFIG), testClass.evaluate_tiled_frames(model, frames, spec, WCONFIG, ensemble=ens), 2)


def test_frame_windows(model, frames):
    w = FrameWindowSpec(3, 2)
    _same(predict(model, frames, InferenceOptions(windows=w), WCONFIG), testClass.evaluate_windowed_frames(model, frames, w, WCONFIG), 2)


def test_frame_windows_tiles_and_ensemble(model, frames):
    w, spec, ens = FrameWindowSpec(2), TileSpec(8), EnsembleSpec("d8")
    got = predict(model, frames[:1], InferenceOptions(ensemble=ens, tiles=spec, windows=w, weights="ema"), WCONFIG)     # the weights are load_model's
    _same(got, testClass.evaluate_windowed_frames(model, frames[:1], w, WCONFIG, tiles=spec, ensemble=ens), 1)
