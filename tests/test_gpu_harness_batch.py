"""The batched directory harness on the device (run with `-m gpu`): the batch letterbox and the
panel pack against the one-image ops they replace, bit for bit, and the pipeline's files
against a reference composed from the existing public ops for the batches plan_batches forms."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]

DEV = "cuda"
SUFFIXES = ("enhanced", "illumination", "comparison")


# ---------------------------------------------------------------------------
# 1. batch letterbox == single letterbox
# ---------------------------------------------------------------------------
def _sources(shapes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]


def _check_letterbox_batch(images, new_shape):
    from utils.letterbox import letterbox_u8_batch, letterbox_u8_image
    ref = torch.stack([letterbox_u8_image(a, new_shape, auto=True, scaleup=False, device=DEV)[0] for a in images])
    out = letterbox_u8_batch(images, new_shape, auto=True, scaleup=False, device=DEV)
    assert out.dtype == torch.float32 and out.shape == ref.shape
    assert torch.equal(out, ref)
    half = letterbox_u8_batch(images, new_shape, auto=True, scaleup=False, device=DEV, dtype=torch.float16)
    assert half.dtype == torch.float16 and torch.equal(half, ref.half())


def test_letterbox_batch_ragged_sources_bitwise():
    from utils.letterbox import letterbox_shape
    shapes = [(128, 96), (100, 100), (64, 64), (40, 64)]  # resized + side borders, resized, identity, row borders
    for s in shapes:
        assert letterbox_shape(s, 64, auto=True, scaleup=False) == (64, 64)
    _check_letterbox_batch(_sources(shapes, 1), 64)


def test_letterbox_batch_identity_misaligned_rows_bitwise():
    # Wo % 4 == 2, odd row count: every other row starts 8 bytes off a 16-byte line, a scalar tail per row
    _check_letterbox_batch(_sources([(37, 50)] * 3, 2), (37, 50))


def test_letterbox_batch_refuses_mixed_shapes():
    from utils.letterbox import letterbox_u8_batch
    images = _sources([(64, 64), (64, 64), (32, 64)], 3)
    with pytest.raises(ValueError, match=r"\[2\]"):
        letterbox_u8_batch(images, 64, device=DEV)


# ---------------------------------------------------------------------------
# 2. panel pack == to_u8_hwc + cat
# ---------------------------------------------------------------------------
def _panel_inputs(B, C, H, W, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(B, C, H, W, generator=g)
    flat = t.view(-1)
    k = torch.arange(256, dtype=torch.float32) / 255.0
    edges = torch.cat([k, torch.nextafter(k, torch.tensor(2.0)), torch.nextafter(k, torch.tensor(-1.0))])
    special = torch.cat([torch.tensor([-0.5, 1.5, float("nan"), 1.0, 0.0]), edges])
    pos = torch.randperm(flat.numel(), generator=g)[:special.numel()]
    flat[pos] = special[:pos.numel()]
    return t.to(dtype).to(DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("hw", [(16, 32), (5, 13), (8, 18)])
def test_panels_u8_bitwise(hw, dtype):
    from upr import runtime
    B, (H, W) = 3, hw
    x, enh = _panel_inputs(B, 3, H, W, dtype, 10), _panel_inputs(B, 3, H, W, dtype, 11)
    illu = _panel_inputs(B, 1, H, W, dtype, 12)
    ref_x = torch.stack([runtime.to_u8_hwc(t) for t in x])
    ref_e = torch.stack([runtime.to_u8_hwc(t) for t in enh])
    ref_i = torch.stack([runtime.to_u8_hwc(t) for t in illu])
    assert int((ref_e == 0).sum()) > 0 and int((ref_e == 255).sum()) > 0
    for with_illu in (False, True):
        for comparison in (None, 2, 3):
            if comparison == 3 and not with_illu:
                with pytest.raises(ValueError):
                    runtime.panels_u8(x, enh, None, comparison=3)
                continue
            e8, i8, c8 = runtime.panels_u8(x, enh, illu if with_illu else None, comparison=comparison)
            assert torch.equal(e8, ref_e)
            assert (i8 is None) == (not with_illu)
            if with_illu:
                assert torch.equal(i8, ref_i)
            if comparison is None:
                assert c8 is None
            else:
                panels = [ref_x, ref_e] + ([ref_i] if comparison == 3 else [])
                assert c8.shape == (B, H, comparison * W, 3)
                assert torch.equal(c8, torch.cat(panels, dim=2))


# ---------------------------------------------------------------------------
# 3-5. the pipeline
# ---------------------------------------------------------------------------
PIPE_SHAPES = [(64, 96)] * 2 + [(96, 64)] + [(64, 96)] + [(32, 32)] + [(64, 96)] + [(96, 64)]  # 4 + 2 + 1, interleaved


@pytest.fixture(scope="module")
def pipe_dir(tmp_path_factory):
    src = tmp_path_factory.mktemp("harness_batch_in")
    rng = np.random.default_rng(5)
    for k, (h, w) in enumerate(PIPE_SHAPES):
        Image.fromarray((rng.integers(0, 256, (h, w, 3)) * 0.4).astype(np.uint8)).save(src / f"im{k}.png")
    return src


def _plain_model():
    from models.model import UP_Retinex
    torch.manual_seed(0)
    return UP_Retinex(use_preact=False, use_aspp=False).to(DEV).eval()


def _composed_reference(files, batch_size, precision, clahe, panels, model):
    """name -> {suffix: u8 HWC pixels on the device}, from the existing ops, batch by batch as planned."""
    from enhancers.adaptive_params import AdaptiveParameterAdjuster
    from enhancers.simple_enhance import letterboxed_shapes, load_image, plan_batches
    from upr import runtime
    ref = {}
    for idxs in plan_batches(letterboxed_shapes(files), batch_size):
        x = torch.cat([load_image(files[i], device=DEV)[0] for i in idxs])
        if precision == "fp16":
            x = x.half()
        with torch.no_grad():
            enh, _, illu = model(x)
        if clahe:
            enh = AdaptiveParameterAdjuster().apply_clahe_enhancement(enh)
        for b, i in enumerate(idxs):
            p = [runtime.to_u8_hwc(x[b]), runtime.to_u8_hwc(enh[b]), runtime.to_u8_hwc(illu[b])]
            name = os.path.splitext(os.path.basename(files[i]))[0]
            ref[name] = {"enhanced": p[1], "illumination": p[2], "comparison": torch.cat(p[:panels], dim=1)}
    return ref


_REFS = {}


def _pipeline_reference(files, precision):
    if precision not in _REFS:
        _REFS[precision] = _composed_reference(files, 4, precision, True, 2, _plain_model())
    return _REFS[precision]


@pytest.mark.parametrize("encoder,precision", [("host", "fp32"), ("device", "fp32"), ("device_lz", "fp32"),
                                               ("device", "fp16")])
def test_pipeline_equals_composed_reference(pipe_dir, tmp_path, encoder, precision):
    from enhancers.simple_enhance import _DEVICE_MATCHES, enhance_batch_images, list_images
    from upr import png
    files = list_images(str(pipe_dir))
    assert len(files) == 7
    out = tmp_path / "out"
    enhance_batch_images(str(pipe_dir), str(out), DEV, use_preact=False, use_aspp=False, seed=0, precision=precision,
                         png_encoder=encoder, batch_size=4)
    assert sorted(os.listdir(out)) == sorted(f"im{k}_{s}.png" for k in range(7) for s in SUFFIXES)  # all 21
    ref = _pipeline_reference(files, precision)
    for name, per in ref.items():
        for suffix, pix in per.items():
            path = out / f"{name}_{suffix}.png"
            np.testing.assert_array_equal(np.asarray(Image.open(path)), pix.cpu().numpy(), err_msg=path.name)
            if encoder in _DEVICE_MATCHES:
                assert open(path, "rb").read() == png.encode(pix, matches=_DEVICE_MATCHES[encoder])[0], path.name


def test_batch_size_one_is_the_default_path(pipe_dir, tmp_path):
    from enhancers.simple_enhance import enhance_batch_images
    kw = dict(use_preact=False, use_aspp=False, seed=0)
    enhance_batch_images(str(pipe_dir), str(tmp_path / "default"), DEV, **kw)
    enhance_batch_images(str(pipe_dir), str(tmp_path / "one"), DEV, batch_size=1, **kw)
    names = sorted(os.listdir(tmp_path / "default"))
    assert len(names) == 21 and names == sorted(os.listdir(tmp_path / "one"))
    for n in names:
        assert open(tmp_path / "default" / n, "rb").read() == open(tmp_path / "one" / n, "rb").read(), n


def test_predict_mode_batched(tmp_path):
    import main as cli
    from enhancers.simple_enhance import list_images
    src = tmp_path / "in"
    src.mkdir()
    rng = np.random.default_rng(9)
    for k in range(3):
        Image.fromarray((rng.integers(0, 256, (64, 64, 3)) * 0.4).astype(np.uint8)).save(src / f"p{k}.png")
    model = _plain_model()
    ckpt = str(tmp_path / "m.pth")
    torch.save({"model_state_dict": model.state_dict()}, ckpt)
    base = ["--mode", "predict", "--checkpoint", ckpt, "--input_path", str(src), "--device", DEV, "--infer_batch", "3"]
    cli.main(base + ["--output_dir", str(tmp_path / "out")])
    ref = _composed_reference(list_images(str(src)), 3, "fp32", False, 3, model)
    assert sorted(os.listdir(tmp_path / "out")) == sorted(f"p{k}_{s}.png" for k in range(3) for s in SUFFIXES)
    for name, per in ref.items():
        for suffix, pix in per.items():
            got = np.asarray(Image.open(tmp_path / "out" / f"{name}_{suffix}.png"))
            np.testing.assert_array_equal(got, pix.cpu().numpy(), err_msg=f"{name}_{suffix}")
        assert per["comparison"].shape == (64, 3 * 64, 3)
    cli.main(base + ["--output_dir", str(tmp_path / "nocmp"), "--no_comparison"])
    assert sorted(os.listdir(tmp_path / "nocmp")) == sorted(f"p{k}_{s}.png" for k in range(3) for s in SUFFIXES[:2])


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_batched_files_equal_one_at_a_time_files(pipe_dir, tmp_path, precision):
    """The forward's outputs were measured not to depend on the batch an image is in (DESIGN.md
    "Batched directory harness": no output byte differed, plain and preact+ASPP, fp32 and fp16, at
    these shapes and at 32 x 512^2), so the batched path writes the one-at-a-time path's pixels."""
    from enhancers.simple_enhance import enhance_batch_images
    kw = dict(use_preact=False, use_aspp=False, seed=0, precision=precision)
    enhance_batch_images(str(pipe_dir), str(tmp_path / "one"), DEV, **kw)
    enhance_batch_images(str(pipe_dir), str(tmp_path / "four"), DEV, batch_size=4, **kw)
    names = sorted(os.listdir(tmp_path / "one"))
    assert len(names) == 21 and names == sorted(os.listdir(tmp_path / "four"))
    for n in names:
        a, b = np.asarray(Image.open(tmp_path / "one" / n)), np.asarray(Image.open(tmp_path / "four" / n))
        np.testing.assert_array_equal(a, b, err_msg=n)
