"""HED edge detector, CPU side: the torch restatement (tests/hed_ref.py) against the reference Network's own outputs
(tests/golden/hed.npz, make_golden_hed.py), the parameter inventory, the state-dict key mapping and the detector's uint8 end."""
import json
import os
import re

import numpy as np
import pytest

from prompt_diffusion_amd import annotators as A
from prompt_diffusion_amd import engine as E
from prompt_diffusion_amd import weights as W
from tests import hed_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def relerr(a, b):
    return float(np.abs(np.asarray(a) - b).max() / (np.abs(b).max() + 1e-30))


def images_from_key(key, shape):   # tests/golden/make_golden_hed.py
    return np.random.Generator(np.random.Philox(key=[79, int(key)])).uniform(0.0, 1.0, shape).astype(np.float32)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "hed.npz"))


@pytest.fixture(scope="module")
def sd():
    return W.synth_hed_state_dict()


@pytest.mark.parametrize("tag", ["tiny", "nonsq", "mid"])
def test_restatement_reproduces_the_reference(fx, sd, tag):
    x = fx[tag + "_images"] if tag + "_images" in fx else images_from_key(int(fx["mid_key"]), (1, 3, 128, 128))
    sides, edge = hed_ref.detect_rgb(sd, x)
    assert sides.shape == fx[tag + "_sides"].shape and edge.shape == fx[tag + "_edge"].shape
    for i in range(5):
        assert relerr(sides[:, i], fx[tag + "_sides"][:, i]) <= 1e-5, i
    assert relerr(edge, fx[tag + "_edge"]) <= 1e-5


def test_fixture_can_see_an_error(fx):
    """What the generator asserts: an unsaturated sigmoid and five side maps of comparable size."""
    for tag in ("tiny", "nonsq", "mid"):
        e, s = fx[tag + "_edge"], fx[tag + "_sides"]
        assert ((e > 0.02) & (e < 0.98)).mean() >= 0.95
        stds = [float(s[:, i].std()) for i in range(5)]
        assert min(stds) >= 0.25 * max(stds)


def test_spec_equals_the_reference_inventory(fx):
    inv = json.loads(str(fx["spec"]))
    assert len(inv) == 38
    assert [("hed." + n, tuple(s)) for n, s in inv] == [(n, tuple(s)) for n, s, _ in W.hed_spec()]
    assert sum(int(np.prod(s)) for _, s, _ in W.hed_spec()) == 14716171


def test_synth_recipe():
    sd = W.synth_hed_state_dict(1234)
    for n, s, k in W.hed_spec():
        base = W.synth_tensor(n, s, k, 1234)
        gain = np.float32(np.sqrt(2.0)) if (".netVgg" in n and k == "w") else np.float32(0.02) if (".netScore" in n and k == "w") else np.float32(1)
        np.testing.assert_array_equal(sd[n], base * gain)


def test_load_hed_state_dict_key_mapping(sd):
    """module..., net... and hed.net... keys land on the same registry names; anything else is refused."""
    class Recorder(E.Engine):
        def __init__(self):      # no library, no GPU: only the key mapping is under test
            self.loaded = []

        def load_tensor(self, name, array):
            self.loaded.append(name)

        def close(self):
            pass

    names = [n for n, _, _ in W.hed_spec()]
    for style in (lambda n: n, lambda n: n[len("hed."):], lambda n: "module" + n[len("hed.net"):]):
        r = Recorder()
        r.load_hed_state_dict({style(n): sd[n] for n in names})
        assert r.loaded == names
    assert W.hed_key("moduleScoreFiv.bias") == W.hed_key("netScoreFiv.bias") == "hed.netScoreFiv.bias"
    for bad in ("netVggSix.0.weight", "hed.netVggOne.1.weight", "first_stage_model.encoder.conv_in.weight", "moduleCombine.weight"):
        with pytest.raises(E.PdError, match="not a HED tensor"):
            Recorder().load_hed_state_dict({bad: np.zeros(1, np.float32)})


def test_detector_postprocessing_truncates_like_the_reference():
    """(edge * 255.0).clip(0, 255).astype(np.uint8): float32 product, truncation."""
    g = np.random.default_rng(5)
    edge = g.uniform(0, 1, (2, 1, 32, 48)).astype(np.float32)
    edge[0, 0, 0, :6] = [0.0, 1.0, 0.999, 1.0 / 255.0, np.nextafter(np.float32(2.0 / 255.0), np.float32(0)), 254.999 / 255.0]
    seen = {}

    class Stub:
        def hed(self, images, what="edge"):
            seen["images"], seen["what"] = images, what
            return edge

    img = g.integers(0, 256, (2, 32, 48, 3), dtype=np.uint8)
    det = A.HEDdetector(Stub())
    out = det.detect(img)
    want = (edge[:, 0] * 255.0).clip(0, 255).astype(np.uint8)       # annotator/hed/__init__.py:113
    assert out.dtype == np.uint8 and out.shape == (2, 32, 48)
    np.testing.assert_array_equal(out, want)
    assert list(out[0, 0, :6]) == [0, 255, 254, 1, 1, 254]
    assert (out != np.rint(edge[:, 0] * 255.0)).any()                   # rounding would differ: this is truncation
    # the engine is handed RGB NCHW float32 in [0, 1] = uint8 / 255 in float32; the BGR flip is the engine's
    assert seen["what"] == "edge" and seen["images"].dtype == np.float32
    np.testing.assert_array_equal(seen["images"], img.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0))
    one = det(img[1])
    np.testing.assert_array_equal(one, want[0])   # the stub returns map 0 for whatever single image it gets
    np.testing.assert_array_equal(hed_ref.to_uint8(edge[:, 0]), want)


def test_hwc3_and_resize_image():
    g = np.random.default_rng(6)
    grey = g.integers(0, 256, (5, 7), dtype=np.uint8)
    assert A.HWC3(grey).shape == (5, 7, 3) and (A.HWC3(grey)[:, :, 1] == grey).all()
    rgba = g.integers(0, 256, (5, 7, 4), dtype=np.uint8)
    c, a = rgba[:, :, :3].astype(np.float32), rgba[:, :, 3:4].astype(np.float32) / 255.0
    np.testing.assert_array_equal(A.HWC3(rgba), (c * a + 255.0 * (1.0 - a)).clip(0, 255).astype(np.uint8))
    img = g.integers(0, 256, (100, 150, 3), dtype=np.uint8)
    assert A.resize_image(img, 256).shape == (256, 384, 3)      # k = 2.56: 256 x 384
    assert A.resize_image(img, 64).shape == (64, 128, 3)        # 64 x 96 -> round(1.5) = 2 (banker's: 96 / 64 = 1.5 -> 2)


def test_exports_and_package_surface():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pdengine.h")).read(), flags=re.S)
    for n in ("pd_hed_configure", "pd_hed_weights_missing", "pd_hed_detect"):
        assert n in E.EXPORTS and re.search(r"\b" + n + r"\s*\(", hdr)
    assert "PD_HED_EDGE  0" in hdr and "PD_HED_SIDES 1" in hdr and (E.PD_HED_EDGE, E.PD_HED_SIDES) == (0, 1)
    import prompt_diffusion_amd as P
    assert P.HEDdetector is A.HEDdetector
    assert W.ModelConfig().hed is False
