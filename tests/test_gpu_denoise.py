"""The illumination-weighted non-local means on the device (run with `-m gpu`):
upr_denoise_nlm_u8's pixels against the numpy restatement byte for byte, and the files of
the harness with denoise="nlm" against the restatement applied to the `off` run's files."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import GOLDEN, has_gpu
import denoise_ref as D
import guided_ref as G

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]

DEV = "cuda"
SUFFIXES = ("enhanced", "illumination", "comparison")


def _g4():
    return np.load(os.path.join(GOLDEN, "g4_real_crop.npz"))["img_u8"]


def _noisy(low_u8, seed=5):
    """A stand-in for an enhanced image: a per-channel gamma curve plus +-6 levels of noise."""
    rng = np.random.default_rng(seed)
    t = 255.0 * (low_u8.astype(np.float64) / 255.0) ** np.array([0.55, 0.6, 0.7]) * 1.05
    return np.clip(np.rint(t + rng.integers(-6, 7, low_u8.shape)), 0, 255).astype(np.uint8)


def _map(h, w, seed=0):
    """A map that holds every level 0..255: a ramp along x, rotated by a few pixels per row."""
    ramp = np.rint(np.linspace(0, 255, w)).astype(np.uint8)
    return np.stack([np.roll(ramp, (3 * y + seed) % w) for y in range(h)])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sources():
    """name -> (u8 HWC image the filter runs on, content rectangle or None)."""
    g4 = _g4()
    out = {}
    for name, src, want in (("77x93", g4[:77, :93], (5, 0, 53, 64)),     # padded rows, content 53 x 64
                            ("5x128", g4[60:65, :], (15, 0, 2, 64)),     # shorter than the patch and the search
                            ("128x74", g4[:, 20:94], (0, 13, 64, 37))):  # left 13, odd width
        low, rect = G.lowres(src, 64)
        assert rect == want, (name, rect)
        out[name] = (_noisy(low), rect)
    out["70x70"] = (_noisy(np.ascontiguousarray(g4[:70, :70])), None)  # partial tiles on both axes
    out["40x56"] = (np.random.default_rng(11).integers(0, 256, (40, 56, 3), dtype=np.uint8), None)
    return out


_SOURCES = {}


def _source(name):
    if not _SOURCES:
        _SOURCES.update(_sources())
    return _SOURCES[name]


def _assert_bytes(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} bytes differ, first at {np.argwhere(bad)[0]}, max |d| " \
                          f"{np.abs(got.astype(int) - want.astype(int)).max()}"


# ---------------------------------------------------------------------------
# 1. the operator
# ---------------------------------------------------------------------------
# (strength, floor, map: None / 1 (u8 [H,W]) / 3 (u8 [H,W,3], channels 1 and 2 hold other values))
VARIANTS = [(1.0, 16, 3), (8.0, 1, 1), (0.0, 16, 3), (1.0, 16, None), (8.0, 16, 1)]


@pytest.mark.parametrize("search,patch", [(1, 1), (5, 2), (10, 3)])
@pytest.mark.parametrize("name", ["77x93", "5x128", "128x74", "70x70", "40x56"])
def test_bytes_equal_the_restatement(name, search, patch):
    from upr import denoise
    img, rect = _source(name)
    m = _map(*img.shape[:2])
    assert m.min() == 0 and m.max() == 255
    m3 = np.stack([m, 255 - m, np.roll(m, 5, axis=1)], axis=2)
    for strength, floor, kind in VARIANTS:
        illu = {None: None, 1: m, 3: m3}[kind]
        got = denoise.nlm(_dev(img)[None], None if illu is None else _dev(illu)[None], rect, strength, floor, search,
                          patch)
        want = D.nlm(img, illu, rect, strength, floor, search, patch)
        _assert_bytes(got[0], want, f"{name} S={search} P={patch} strength={strength} floor={floor} map={kind}")
        if strength == 0.0:
            _assert_bytes(got[0], img, f"{name} strength 0 is the identity")


def test_defaults_and_a_constant_image():
    from upr import denoise
    img, rect = _source("77x93")
    _assert_bytes(denoise.nlm(_dev(img)[None])[0], D.nlm(img), "defaults")
    flat = np.full((70, 70, 3), 97, np.uint8)
    flat[..., 2] = 200
    _assert_bytes(denoise.nlm(_dev(flat)[None], _dev(_map(70, 70))[None], None, 8.0)[0], flat, "constant image")


def test_batch_of_three_equals_single_runs():
    from upr import denoise
    img, rect = _source("77x93")
    imgs = np.stack([img, img[::-1], _noisy(np.roll(img, 7, axis=1), 9)])
    maps = np.stack([_map(64, 64, k) for k in range(3)])
    got = denoise.nlm(_dev(imgs), _dev(maps), rect, 2.0)
    for b in range(3):
        one = denoise.nlm(_dev(imgs[b])[None], _dev(maps[b])[None], rect, 2.0)
        assert torch.equal(got[b], one[0])
        _assert_bytes(got[b], D.nlm(imgs[b], maps[b], rect, 2.0), f"image {b}")


def test_bars_are_copied_and_never_mixed_in():
    from upr import denoise
    for name in ("77x93", "128x74", "5x128"):
        img, rect = _source(name)
        top, left, nh, nw = rect
        bars = np.full_like(img, 255)
        bars[top:top + nh, left:left + nw] = img[top:top + nh, left:left + nw]
        got = denoise.nlm(_dev(bars)[None], None, rect, 8.0)[0].cpu().numpy()
        inside = np.zeros(img.shape[:2], bool)
        inside[top:top + nh, left:left + nw] = True
        np.testing.assert_array_equal(got[~inside], bars[~inside])
        want = D.nlm(img, None, rect, 8.0)
        np.testing.assert_array_equal(got[inside], want[inside])


def test_reruns_are_identical():
    from upr import denoise
    img, _ = _source("70x70")
    x, m = _dev(img)[None], _dev(_map(70, 70))[None]
    first = denoise.nlm(x, m, None, 4.0)
    for _ in range(3):
        assert torch.equal(denoise.nlm(x, m, None, 4.0), first)


def test_refused_arguments():
    from upr import denoise
    img, rect = _source("77x93")
    x = _dev(img)[None]
    with pytest.raises(ValueError):
        denoise.nlm(x, out=x)  # aliased
    both = torch.empty(2 * x.numel() - 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):  # two tensors that share all but one pixel
        denoise.nlm(both[:x.numel()].view(x.shape), out=both[x.numel() - 3:].view(x.shape))
    with pytest.raises(RuntimeError):
        denoise.nlm(torch.from_numpy(img)[None])  # a CPU tensor
    with pytest.raises(RuntimeError):
        denoise.nlm(x, torch.from_numpy(_map(64, 64))[None])
    for bad in ((30, 0, 40, 64), (0, 1, 64, 64), (-1, 0, 10, 10), (0, 0, 0, 10)):
        with pytest.raises(ValueError):
            denoise.nlm(x, None, bad)
    with pytest.raises(ValueError):
        denoise.nlm(x, _dev(_map(64, 32))[None])
    with pytest.raises(ValueError):
        denoise.nlm(x, search=11)
    out = torch.empty_like(x)
    assert denoise.nlm(x, None, rect, out=out) is out
    _assert_bytes(out[0], D.nlm(img, None, rect), "out=")


# ---------------------------------------------------------------------------
# 2. the harness
# ---------------------------------------------------------------------------
KW = dict(use_preact=False, use_aspp=False, seed=0)
NLM = dict(denoise="nlm", denoise_strength=2.0)


@pytest.fixture(scope="module")
def pipe(tmp_path_factory):
    """The input directory, its sources, and the files of a max_size 64 run with denoise off."""
    from enhancers.simple_enhance import enhance_batch_images
    root = tmp_path_factory.mktemp("denoise")
    src = root / "in"
    src.mkdir()
    g4 = _g4()
    images = {"a77": g4[:77, :93], "b77": g4[51:, 35:], "c128": g4, "d40": g4[:40, :40]}
    for k, a in images.items():
        assert a.shape[:2] in ((77, 93), (128, 128), (40, 40))
        Image.fromarray(np.ascontiguousarray(a)).save(src / f"{k}.png")
    enhance_batch_images(str(src), str(root / "off"), DEV, max_size=64, **KW)
    off = {n: {s: np.asarray(Image.open(root / "off" / f"{n}_{s}.png")) for s in SUFFIXES} for n in images}
    want = {}
    for n, a in images.items():  # the restatement on the off run's files
        rect = G.content_rect(a.shape[:2], 64)
        want[n] = D.nlm(off[n]["enhanced"], off[n]["illumination"], rect, strength=2.0)
        assert (want[n] != off[n]["enhanced"]).any()
    return root, src, images, off, want


@pytest.mark.parametrize("encoder", ["host", "device"])
def test_files_equal_the_restatement_on_the_off_files(pipe, tmp_path, encoder):
    from enhancers.simple_enhance import enhance_batch_images
    root, src, images, off, want = pipe
    for bs in (1, 4):
        enhance_batch_images(str(src), str(tmp_path / str(bs)), DEV, max_size=64, batch_size=bs, png_encoder=encoder,
                             **KW, **NLM)
    names = sorted(f"{n}_{s}.png" for n in images for s in SUFFIXES)
    for bs in (1, 4):
        out = tmp_path / str(bs)
        assert sorted(os.listdir(out)) == names
        for n in images:
            got = {s: np.asarray(Image.open(out / f"{n}_{s}.png")) for s in SUFFIXES}
            Wl = want[n].shape[1]
            np.testing.assert_array_equal(got["enhanced"], want[n], err_msg=f"{n} enhanced, batch {bs}")
            np.testing.assert_array_equal(got["comparison"][:, Wl:], want[n], err_msg=f"{n} panel, batch {bs}")
            np.testing.assert_array_equal(got["comparison"][:, :Wl], off[n]["comparison"][:, :Wl])
            np.testing.assert_array_equal(got["illumination"], off[n]["illumination"])
            if encoder == "host":  # the same encoder as the off run: the very file
                assert open(out / f"{n}_illumination.png", "rb").read() == \
                    open(root / "off" / f"{n}_illumination.png", "rb").read()
    for f in names:  # batch 1 and batch 4 write identical files
        assert open(tmp_path / "1" / f, "rb").read() == open(tmp_path / "4" / f, "rb").read(), f


def test_original_size_files(pipe, tmp_path):
    from enhancers.simple_enhance import enhance_batch_images
    root, src, images, off, want = pipe
    for bs in (1, 4):
        enhance_batch_images(str(src), str(tmp_path / str(bs)), DEV, max_size=64, batch_size=bs,
                             output_size="original", **KW, **NLM)
    names = sorted(f"{n}_{s}.png" for n in images for s in SUFFIXES)
    assert sorted(os.listdir(tmp_path / "1")) == names == sorted(os.listdir(tmp_path / "4"))
    for n, a in images.items():
        H, W = a.shape[:2]
        for s in SUFFIXES:
            assert Image.open(tmp_path / "1" / f"{n}_{s}.png").size == ((2 if s == "comparison" else 1) * W, H)
    for f in names:
        assert open(tmp_path / "1" / f, "rb").read() == open(tmp_path / "4" / f, "rb").read(), f
    # nothing was resized for the 40 x 40 image: the content crop of the denoised letterboxed pixels
    top, left, nh, nw = G.content_rect((40, 40), 64)
    np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "1" / "d40_enhanced.png")),
                                  want["d40"][top:top + nh, left:left + nw])
    # the resized ones: the restore of the denoised target
    lb = off["a77"]
    rect = G.content_rect((77, 93), 64)
    ref = G.restore(np.ascontiguousarray(images["a77"]), lb["comparison"][:, :64], want["a77"], lb["illumination"],
                    rect, comparison=2)
    for s, w in zip(SUFFIXES, ref):
        np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "1" / f"a77_{s}.png")), w, err_msg=s)


@pytest.mark.parametrize("encoder", ["host", "device"])
def test_jpeg_files_decode_at_the_right_size(pipe, tmp_path, encoder):
    from enhancers.simple_enhance import enhance_batch_images
    _, src, images, off, _ = pipe
    enhance_batch_images(str(src), str(tmp_path), DEV, max_size=64, batch_size=4, png_encoder=encoder,
                         image_format="jpg", **KW, **NLM)
    assert sorted(os.listdir(tmp_path)) == sorted(f"{n}_{s}.jpg" for n in images for s in SUFFIXES)
    for n in images:
        Hl, Wl = off[n]["enhanced"].shape[:2]
        for s in SUFFIXES:
            im = Image.open(tmp_path / f"{n}_{s}.jpg")
            im.load()
            assert im.size == ((2 if s == "comparison" else 1) * Wl, Hl)


def test_denoise_off_is_the_default_path(pipe, tmp_path):
    from enhancers.simple_enhance import enhance_batch_images
    root, src, images, _, _ = pipe
    enhance_batch_images(str(src), str(tmp_path / "kw1"), DEV, max_size=64, denoise="off", denoise_strength=8.0, **KW)
    enhance_batch_images(str(src), str(tmp_path / "kw4"), DEV, max_size=64, batch_size=4, denoise="off", **KW)
    enhance_batch_images(str(src), str(tmp_path / "plain4"), DEV, max_size=64, batch_size=4, **KW)
    for a, b in ((root / "off", tmp_path / "kw1"), (tmp_path / "plain4", tmp_path / "kw4")):
        names = sorted(os.listdir(a))
        assert len(names) == 12 and names == sorted(os.listdir(b))
        for n in names:
            assert open(a / n, "rb").read() == open(b / n, "rb").read(), n


@pytest.mark.parametrize("enhancer", ["adaptive", "multi_scale", "content_aware"])
def test_single_image_path_for_every_enhancer(pipe, tmp_path, enhancer):
    from enhancers.simple_enhance import enhance_single_image, load_image
    from models.model import UP_Retinex
    from upr import runtime
    _, src, images, _, _ = pipe
    torch.manual_seed(0)
    model = UP_Retinex(use_preact=False, use_aspp=False).to(DEV).eval()
    path = str(src / "a77.png")
    enh, illu = enhance_single_image(model, path, str(tmp_path), DEV, max_size=64,
                                     enable_multi_scale=enhancer == "multi_scale",
                                     enable_content_aware=enhancer == "content_aware", **NLM)
    assert enh.shape == (1, 3, 64, 64) and illu.shape[2:] == (64, 64)  # the tensors, as before
    x, _ = load_image(path, 64, device=DEV)
    low, tgt, ill = (runtime.to_u8_hwc(t[0]).cpu().numpy() for t in (x, enh, illu))
    want = D.nlm(tgt, ill, (5, 0, 53, 64), strength=2.0)
    assert (want != tgt).any()
    np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "a77_enhanced.png")), want)
    np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "a77_illumination.png")), ill)
    np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "a77_comparison.png")),
                                  np.concatenate([low, want], axis=1))


def test_predict_mode(pipe, tmp_path):
    import main as cli
    from models.model import UP_Retinex
    _, src, images, _, _ = pipe
    torch.manual_seed(0)
    model = UP_Retinex(use_preact=False, use_aspp=False)
    ckpt = str(tmp_path / "m.pth")
    torch.save({"model_state_dict": model.state_dict()}, ckpt)
    base = ["--mode", "predict", "--checkpoint", ckpt, "--input_path", str(src), "--device", DEV, "--max_size", "64"]
    cli.main(base + ["--output_dir", str(tmp_path / "off")])
    nlm = ["--denoise", "nlm", "--denoise_strength", "2", "--denoise_search", "3", "--denoise_patch", "1",
           "--denoise_floor", "32"]
    for tag, extra in (("loop", []), ("batched", ["--infer_batch", "4"])):
        out = tmp_path / tag
        cli.main(base + ["--output_dir", str(out)] + nlm + extra)
        assert sorted(os.listdir(out)) == sorted(f"{n}_{s}.png" for n in images for s in SUFFIXES)
        for n, a in images.items():
            off = {s: np.asarray(Image.open(tmp_path / "off" / f"{n}_{s}.png")) for s in SUFFIXES}
            want = D.nlm(off["enhanced"], off["illumination"], G.content_rect(a.shape[:2], 64), 2.0, 32, 3, 1)
            Wl = want.shape[1]
            cmp = np.asarray(Image.open(out / f"{n}_comparison.png"))
            np.testing.assert_array_equal(np.asarray(Image.open(out / f"{n}_enhanced.png")), want, err_msg=f"{tag} {n}")
            np.testing.assert_array_equal(cmp[:, Wl:2 * Wl], want)
            np.testing.assert_array_equal(cmp[:, :Wl], off["comparison"][:, :Wl])
            np.testing.assert_array_equal(cmp[:, 2 * Wl:], off["illumination"])
            np.testing.assert_array_equal(np.asarray(Image.open(out / f"{n}_illumination.png")), off["illumination"])
