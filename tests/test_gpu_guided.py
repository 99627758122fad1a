"""The guided-filter restore on the device (run with `-m gpu`): upr_guided_fit's coefficients
against the numpy restatement bit for bit, upr_guided_apply's outputs byte for byte, and the
original-size files of the harness against the restatement applied to the letterboxed files."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import GOLDEN, has_gpu
import guided_ref as G

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]

DEV = "cuda"
SUFFIXES = ("enhanced", "illumination", "comparison")


def _g4():
    return np.load(os.path.join(GOLDEN, "g4_real_crop.npz"))["img_u8"]


def _target(low_u8, seed=5):
    """A stand-in for an enhancement: a per-channel gamma curve plus +-2 levels of noise."""
    rng = np.random.default_rng(seed)
    t = 255.0 * (low_u8.astype(np.float64) / 255.0) ** np.array([0.55, 0.6, 0.7]) * 1.05
    return np.clip(np.rint(t + rng.integers(-2, 3, low_u8.shape)), 0, 255).astype(np.uint8)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sources():
    """name -> (src u8 HWC, max_size, expected content rectangle)."""
    g4 = _g4()
    rng = np.random.default_rng(21)
    return {
        "77x93": (g4[:77, :93], 64, (5, 0, 53, 64)),     # non-integer ratio, padded rows, W % 4 != 0
        "5x128": (g4[60:65, :], 64, (15, 0, 2, 64)),     # the window is taller than the content
        "128x74": (g4[:, 20:94], 64, (0, 13, 64, 37)),   # odd content width, padded columns
        "128x128": (g4, 64, (0, 0, 64, 64)),             # exact 2x
        "480x640": (rng.integers(0, 256, (480, 640, 3), dtype=np.uint8), 64, (8, 0, 48, 64)),  # 10x
    }


_CASES = {}


def _case(name):
    """(src, low, target, illu_lb, rect) of a source, computed once."""
    if name not in _CASES:
        src, ms, want = _sources()[name]
        low, rect = G.lowres(src, ms)
        assert rect == want, (name, rect)
        tgt = _target(low)
        illu = np.repeat(_target(low, 6)[..., 1:2], 3, axis=2)
        _CASES[name] = (np.ascontiguousarray(src), low, tgt, illu, rect)
    return _CASES[name]


def _assert_bits(ab_dev, ref, what):
    got = ab_dev.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.float64
    bad = got.view(np.int64) != ref.view(np.int64)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} coefficients differ, max |d| " \
                          f"{np.abs(got - ref).max():.3e}"


# ---------------------------------------------------------------------------
# 1. fit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("r,eps", [(1, 1e-4), (4, 1e-4), (16, 1e-4), (4, 1e-2), (4, 1e-6)])
@pytest.mark.parametrize("name", ["77x93", "5x128", "128x74"])
def test_fit_bitwise(name, r, eps):
    from upr import guided
    _, low, tgt, _, rect = _case(name)
    ab = guided.fit(_dev(low)[None], _dev(tgt)[None], rect, r, eps)
    assert ab.shape == (1, 2, 3, rect[2], rect[3])
    _assert_bits(ab[0], G.fit(low, tgt, rect, r, eps), f"{name} r={r} eps={eps}")


def test_fit_radius_32_on_128_square():
    from upr import guided
    g4 = _g4()
    tgt, rect = _target(g4), (0, 0, 128, 128)
    ab = guided.fit(_dev(g4)[None], _dev(tgt)[None], rect, 32, 1e-4)
    _assert_bits(ab[0], G.fit(g4, tgt, rect, 32, 1e-4), "r=32")


def test_fit_checkerboard_and_constant_target():
    from upr import guided
    yy, xx = np.mgrid[:64, :64]
    board = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    rect = (5, 0, 53, 64)
    for guide, tgt in ((board, 255 - board), (board, board), (_case("77x93")[1], np.full((64, 64, 3), 97, np.uint8))):
        for r in (1, 4, 16):
            ab = guided.fit(_dev(guide)[None], _dev(tgt)[None], rect, r, 1e-4)
            _assert_bits(ab[0], G.fit(guide, tgt, rect, r, 1e-4), f"r={r}")
    got = ab[0].cpu().numpy()  # the constant target: a = 0, b = the constant, exactly
    assert (got[0] == 0).all() and (got[1] == 97).all()


def test_fit_batch_of_three_equals_single_runs():
    from upr import guided
    _, low, tgt, _, rect = _case("77x93")
    lows = np.stack([low, low[::-1], np.roll(low, 7, axis=1)])
    tgts = np.stack([tgt, _target(low[::-1], 8), np.roll(tgt, 3, axis=0)])
    ab = guided.fit(_dev(lows), _dev(tgts), rect)
    for b in range(3):
        one = guided.fit(_dev(lows[b])[None], _dev(tgts[b])[None], rect)
        assert torch.equal(ab[b].view(torch.int64), one[0].view(torch.int64))
        _assert_bits(ab[b], G.fit(lows[b], tgts[b], rect), f"image {b}")


# ---------------------------------------------------------------------------
# 2. apply
# ---------------------------------------------------------------------------
def _check_apply(outs, refs, what):
    for got, want, kind in zip(outs, refs, SUFFIXES):
        assert (got is None) == (want is None), (what, kind)
        if want is not None:
            g = got.cpu().numpy()
            assert g.shape == want.shape, (what, kind, g.shape, want.shape)
            bad = g != want
            assert not bad.any(), f"{what} {kind}: {int(bad.sum())} bytes differ, first at {np.argwhere(bad)[0]}"


@pytest.mark.parametrize("name", ["77x93", "128x128", "5x128", "480x640", "128x74"])
def test_apply_bytewise(name):
    from upr import guided
    src, low, tgt, illu, rect = _case(name)
    ab = G.fit(low, tgt, rect)
    for with_illu in (False, True):
        for comparison in (None, 2, 3):
            if comparison == 3 and not with_illu:
                with pytest.raises(ValueError):
                    guided.apply(_dev(src)[None], _dev(ab)[None], None, rect, 3)
                continue
            outs = guided.apply(_dev(src)[None], _dev(ab)[None], _dev(illu)[None] if with_illu else None, rect,
                                comparison)
            refs = G.apply(src, ab, illu if with_illu else None, rect, comparison)
            _check_apply([o[0] if o is not None else None for o in outs], refs, f"{name} illu={with_illu} "
                                                                                 f"panels={comparison}")


def test_apply_batch_of_three_at_an_aligned_stride():
    from upr import guided
    from utils.letterbox import StagedSources
    src, low, tgt, illu, rect = _case("77x93")
    srcs = [src, np.ascontiguousarray(src[::-1]), np.ascontiguousarray(src[:, ::-1])]
    lows = [G.lowres(s, 64)[0] for s in srcs]
    tgts = [_target(l, 30 + k) for k, l in enumerate(lows)]
    illus = [np.repeat(_target(l, 40 + k)[..., :1], 3, axis=2) for k, l in enumerate(lows)]
    abs_ = np.stack([G.fit(l, t, rect) for l, t in zip(lows, tgts)])
    n = src.size
    stride = (n + 15) // 16 * 16
    assert stride % 16 == 0 and stride != n and n % 4 != 0
    buf = np.full(3 * stride, 255, np.uint8)
    for b, s in enumerate(srcs):
        buf[b * stride:b * stride + n] = s.reshape(-1)
    staged = StagedSources(_dev(buf), stride, src.shape[:2], 3)
    outs = guided.apply(staged, _dev(abs_), _dev(np.stack(illus)), rect, 3)
    for b in range(3):
        _check_apply([o[b] for o in outs], G.apply(srcs[b], abs_[b], illus[b], rect, 3), f"image {b}")
    dense = guided.apply(_dev(np.stack(srcs)), _dev(abs_), _dev(np.stack(illus)), rect, 3)
    for a, d in zip(outs, dense):
        assert torch.equal(a, d)


def test_restore_equals_restatement_and_crops_without_a_resize():
    from upr import guided
    src, low, tgt, illu, rect = _case("77x93")
    outs = guided.restore(_dev(src)[None], _dev(low)[None], _dev(tgt)[None], _dev(illu)[None], rect, comparison=3)
    _check_apply([o[0] for o in outs], G.restore(src, low, tgt, illu, rect, comparison=3), "restore")
    small = np.ascontiguousarray(_g4()[:40, :40])
    low, rect = G.lowres(small, 64)
    assert rect[2:] == (40, 40)
    tgt = _target(low)
    outs = guided.restore(_dev(small)[None], _dev(low)[None], _dev(tgt)[None], _dev(tgt)[None], rect, comparison=2)
    _check_apply([o[0] if o is not None else None for o in outs], G.restore(small, low, tgt, tgt, rect, comparison=2),
                 "crop")
    with pytest.raises(ValueError):
        guided.fit(_dev(low)[None], _dev(tgt)[None], rect, radius=33)
    with pytest.raises(ValueError):
        guided.fit(_dev(low)[None], _dev(tgt)[None], (30, 0, 40, 40))


# ---------------------------------------------------------------------------
# 3. the harness
# ---------------------------------------------------------------------------
KW = dict(use_preact=False, use_aspp=False, seed=0)


@pytest.fixture(scope="module")
def pipe(tmp_path_factory):
    """The input directory, its sources, and today's (letterboxed) files of a max_size 64 run."""
    from enhancers.simple_enhance import enhance_batch_images
    root = tmp_path_factory.mktemp("guided")
    src = root / "in"
    src.mkdir()
    g4 = _g4()
    images = {"a77": g4[:77, :93], "b77": g4[51:, 35:], "c128": g4, "d40": g4[:40, :40]}
    for k, a in images.items():
        assert a.shape[:2] in ((77, 93), (128, 128), (40, 40))
        Image.fromarray(np.ascontiguousarray(a)).save(src / f"{k}.png")
    enhance_batch_images(str(src), str(root / "letterbox"), DEV, max_size=64, **KW)
    lb = {n: {s: np.asarray(Image.open(root / "letterbox" / f"{n}_{s}.png")) for s in SUFFIXES} for n in images}
    return root, src, images, lb


def _expected(images, lb, comparison=2):
    """name -> {suffix: pixels}: the restatement on the letterboxed files' bytes."""
    out = {}
    for n, src in images.items():
        rect = G.content_rect(src.shape[:2], 64)
        Wl = lb[n]["enhanced"].shape[1]
        outs = G.restore(np.ascontiguousarray(src), lb[n]["comparison"][:, :Wl], lb[n]["enhanced"],
                         lb[n]["illumination"], rect, comparison=comparison)
        out[n] = dict(zip(SUFFIXES, outs))
    return out


@pytest.mark.parametrize("fmt", ["png", "jpg"])
@pytest.mark.parametrize("encoder", ["host", "device"])
@pytest.mark.parametrize("batch_size", [1, 4])
def test_original_size_files(pipe, tmp_path, batch_size, encoder, fmt):
    from enhancers.simple_enhance import enhance_batch_images
    root, src, images, lb = pipe
    out = tmp_path / "out"
    enhance_batch_images(str(src), str(out), DEV, max_size=64, output_size="original", batch_size=batch_size,
                         png_encoder=encoder, image_format=fmt, **KW)
    assert sorted(os.listdir(out)) == sorted(f"{n}_{s}.{fmt}" for n in images for s in SUFFIXES)
    want = _expected(images, lb)
    for n, a in images.items():
        H, W = a.shape[:2]
        for s in SUFFIXES:
            got = np.asarray(Image.open(out / f"{n}_{s}.{fmt}").convert("RGB"))
            assert got.shape == (H, (2 if s == "comparison" else 1) * W, 3), (n, s, got.shape)
            if fmt == "png":
                np.testing.assert_array_equal(got, want[n][s], err_msg=f"{n}_{s}")
    if fmt == "png":  # nothing was resized for the 40 x 40 image: the content crop of the letterboxed files
        top, left, nh, nw = G.content_rect((40, 40), 64)
        for s in SUFFIXES[:2]:
            np.testing.assert_array_equal(np.asarray(Image.open(out / f"d40_{s}.png")),
                                          lb["d40"][s][top:top + nh, left:left + nw])


@pytest.mark.parametrize("fmt", ["png", "jpg"])
def test_batch_one_and_four_write_identical_files(pipe, tmp_path, fmt):
    from enhancers.simple_enhance import enhance_batch_images
    _, src, images, _ = pipe
    for bs in (1, 4):
        enhance_batch_images(str(src), str(tmp_path / str(bs)), DEV, max_size=64, output_size="original",
                             batch_size=bs, image_format=fmt, **KW)
    names = sorted(os.listdir(tmp_path / "1"))
    assert len(names) == 12 and names == sorted(os.listdir(tmp_path / "4"))
    for n in names:
        assert open(tmp_path / "1" / n, "rb").read() == open(tmp_path / "4" / n, "rb").read(), n


def test_letterbox_keyword_writes_todays_files(pipe, tmp_path):
    from enhancers.simple_enhance import enhance_batch_images
    root, src, images, _ = pipe
    for bs in (1, 4):
        enhance_batch_images(str(src), str(tmp_path / f"kw{bs}"), DEV, max_size=64, output_size="letterbox",
                             batch_size=bs, **KW)
    enhance_batch_images(str(src), str(tmp_path / "plain4"), DEV, max_size=64, batch_size=4, **KW)
    for a, b in ((root / "letterbox", tmp_path / "kw1"), (tmp_path / "plain4", tmp_path / "kw4")):
        names = sorted(os.listdir(a))
        assert len(names) == 12 and names == sorted(os.listdir(b))
        for n in names:
            assert open(a / n, "rb").read() == open(b / n, "rb").read(), n


@pytest.mark.parametrize("enhancer", ["adaptive", "multi_scale", "content_aware"])
def test_single_image_path_for_every_enhancer(pipe, tmp_path, enhancer):
    from enhancers.simple_enhance import enhance_single_image, load_image
    from models.model import UP_Retinex
    from upr import runtime
    _, src, images, _ = pipe
    torch.manual_seed(0)
    model = UP_Retinex(use_preact=False, use_aspp=False).to(DEV).eval()
    path = str(src / "a77.png")
    enh, illu = enhance_single_image(model, path, str(tmp_path), DEV, max_size=64, output_size="original",
                                     enable_multi_scale=enhancer == "multi_scale",
                                     enable_content_aware=enhancer == "content_aware")
    assert enh.shape == (1, 3, 64, 64) and illu.shape[2:] == (64, 64)  # the letterboxed tensors, as before
    x, _ = load_image(path, 64, device=DEV)
    low, tgt, ill = (runtime.to_u8_hwc(t[0]).cpu().numpy() for t in (x, enh, illu))
    want = G.restore(np.ascontiguousarray(images["a77"]), low, tgt, ill, (5, 0, 53, 64), comparison=2)
    for s, w in zip(SUFFIXES, want):
        np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / f"a77_{s}.png")), w, err_msg=s)


def test_predict_mode_original_size(pipe, tmp_path):
    import main as cli
    from models.model import UP_Retinex
    _, src, images, _ = pipe
    torch.manual_seed(0)
    model = UP_Retinex(use_preact=False, use_aspp=False)
    ckpt = str(tmp_path / "m.pth")
    torch.save({"model_state_dict": model.state_dict()}, ckpt)
    base = ["--mode", "predict", "--checkpoint", ckpt, "--input_path", str(src), "--device", DEV, "--max_size", "64"]
    cli.main(base + ["--output_dir", str(tmp_path / "lb"), "--infer_batch", "4"])
    lb = {n: {s: np.asarray(Image.open(tmp_path / "lb" / f"{n}_{s}.png")) for s in SUFFIXES} for n in images}
    want = _expected(images, lb, comparison=3)
    for tag, extra in (("loop", []), ("batched", ["--infer_batch", "4"])):
        out = tmp_path / tag
        cli.main(base + ["--output_dir", str(out), "--output_size", "original"] + extra)
        assert sorted(os.listdir(out)) == sorted(f"{n}_{s}.png" for n in images for s in SUFFIXES)
        for n, a in images.items():
            H, W = a.shape[:2]
            assert Image.open(out / f"{n}_comparison.png").size == (3 * W, H)
            for s in SUFFIXES:
                np.testing.assert_array_equal(np.asarray(Image.open(out / f"{n}_{s}.png")), want[n][s],
                                              err_msg=f"{tag} {n}_{s}")
    cli.main(base + ["--output_dir", str(tmp_path / "nocmp"), "--output_size", "original", "--no_comparison",
                     "--input_path", str(src / "a77.png")])
    assert sorted(os.listdir(tmp_path / "nocmp")) == ["a77_enhanced.png", "a77_illumination.png"]
