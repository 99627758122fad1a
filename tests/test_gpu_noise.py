"""Blind denoising on the device (run with `-m gpu`): upr_noise_sigma_u8's sigma against the
numpy restatement bit for bit, upr_denoise_lut_dev's tables entry for entry,
upr_denoise_nlm_u8_luts and nlm_auto byte for byte, and the harness's files with
denoise_strength="auto" against the restatement applied to the `off` run's files."""
import ctypes
import os
import struct

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import GOLDEN, has_gpu
import denoise_ref as D
import guided_ref as G
import noise_ref as N

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]

DEV = "cuda"
SUFFIXES = ("enhanced", "illumination", "comparison")


def _g4():
    return np.load(os.path.join(GOLDEN, "g4_real_crop.npz"))["img_u8"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(x):
    return struct.pack("<d", float(x))


def _noised(img, std, seed):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(img.astype(np.float64) + rng.normal(0.0, std, img.shape)), 0, 255).astype(np.uint8)


def _images():
    """name -> (u8 HWC image, content rectangle or None)."""
    g4 = _g4()
    rng = np.random.default_rng(21)
    out = {"40x56 noise": (rng.integers(0, 256, (40, 56, 3), dtype=np.uint8), None)}
    low, rect = G.lowres(g4[:77, :93], 64)
    assert rect == (5, 0, 53, 64)
    out["77x93 letterboxed"] = (_noised(low, 2.0, 1), rect)
    low, rect = G.lowres(g4[:, 20:94], 64)
    assert rect == (0, 13, 64, 37)  # a left bar of odd width
    out["left bar 13"] = (_noised(low, 1.0, 2), rect)
    out["3 rows"] = (_noised(g4[:64, :64], 3.0, 3), (30, 0, 3, 64))
    out["2 rows"] = (_noised(g4[:64, :64], 3.0, 3), (15, 0, 2, 64))
    out["3 columns"] = (_noised(g4[:64, :64], 3.0, 3), (0, 7, 64, 3))
    flat = np.full((128, 128, 3), 64, np.uint8)
    flat[..., 1] = 200
    out["128x128 constant"] = (flat, None)
    out["extremes"] = (rng.choice(np.array([0, 1, 254, 255], np.uint8), (48, 80, 3)), None)
    out["all zero"] = (np.zeros((20, 20, 3), np.uint8), None)
    # more than one tile on both axes, neither a multiple of the 64-sample tile; odd row pitch
    out["131x199"] = (_noised(np.tile(g4, (2, 2, 1))[:131, :199] // 2 + 20, 4.0, 4), None)
    out["70x67 in 128x131"] = (_noised(np.tile(g4, (1, 2, 1))[:, :131], 0.7, 5), (9, 31, 70, 67))
    out["66x66"] = (_noised(g4[:66, :66], 1.5, 6), None)   # exactly one full tile
    out["67x67"] = (_noised(g4[:67, :67], 1.5, 6), None)   # one sample more on both axes
    return out


_IMAGES = {}


def _image(name):
    if not _IMAGES:
        _IMAGES.update(_images())
    return _IMAGES[name]


NAMES = ["40x56 noise", "77x93 letterboxed", "left bar 13", "3 rows", "2 rows", "3 columns", "128x128 constant",
         "extremes", "all zero", "131x199", "70x67 in 128x131", "66x66", "67x67"]


def _assert_bytes(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} bytes differ, first at {np.argwhere(bad)[0]}"


# ---------------------------------------------------------------------------
# 1. the estimate
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_sigma_bits_equal_the_restatement(name):
    from upr import denoise
    img, rect = _image(name)
    got = denoise.estimate_sigma(_dev(img)[None], rect)
    assert got.dtype == torch.float64 and got.shape == (1,) and got.is_cuda
    want = N.sigma(img, rect)
    print(f"{name}: device {float(got[0])!r} restatement {want!r}")
    assert _bits(got[0]) == _bits(want)
    if name in ("2 rows", "all zero"):
        assert want == 0.0
    elif name != "extremes":
        assert want > 0.0


def test_batch_of_three_equals_single_runs_and_reruns_are_identical():
    from upr import denoise
    g4 = _g4()
    imgs = np.stack([_noised(g4[:90, :101], s, 7 + k) for k, s in enumerate((0.5, 2.0, 6.0))])
    rect = (3, 5, 80, 90)
    x = _dev(imgs)
    got = denoise.estimate_sigma(x, rect)
    want = [N.sigma(a, rect) for a in imgs]
    assert want[0] < want[1] < want[2]
    for b in range(3):
        one = denoise.estimate_sigma(x[b:b + 1], rect)
        assert _bits(one[0]) == _bits(got[b]) == _bits(want[b])
    for _ in range(2):
        assert torch.equal(denoise.estimate_sigma(x, rect), got)


# ---------------------------------------------------------------------------
# 2. the tables
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("scale,floor,patch", [(1.0, 16, 2), (0.5, 1, 1), (8.0, 255, 3)])
def test_device_tables_equal_the_host_table(scale, floor, patch):
    from upr import denoise
    imgs = [_image(n) for n in ("77x93 letterboxed", "2 rows", "left bar 13")]
    sig = torch.cat([denoise.estimate_sigma(_dev(a)[None], r) for a, r in imgs] +
                    [torch.tensor([0.0, 1.0, 1e-200, 3.0350000000000001, 250.0], dtype=torch.float64, device=DEV)])
    back = sig.cpu().tolist()
    assert back[1] == 0.0 and back[3] == 0.0  # a measured and a given sigma of exactly 0
    tables = denoise.lut_device(sig, scale, floor, patch)
    assert tables.shape == (len(back), 256)
    got = tables.cpu().numpy().view(np.uint32)
    for b, s in enumerate(back):
        host = np.ctypeslib.as_array(denoise.lut(scale * s, floor, patch)).astype(np.uint32)
        np.testing.assert_array_equal(got[b], host, err_msg=f"sigma {s!r}")
        np.testing.assert_array_equal(got[b], D.lut(scale * s, floor, patch), err_msg=f"sigma {s!r} (numpy)")
    assert (got[1] == 4294967295).all()


# ---------------------------------------------------------------------------
# 3. the filter with a table per image
# ---------------------------------------------------------------------------
def _enhanced(low, seed=5):
    rng = np.random.default_rng(seed)
    t = 255.0 * (low.astype(np.float64) / 255.0) ** np.array([0.55, 0.6, 0.7]) * 1.05
    return np.clip(np.rint(t + rng.integers(-6, 7, low.shape)), 0, 255).astype(np.uint8)


def _map(h, w, seed=0):
    ramp = np.rint(np.linspace(0, 255, w)).astype(np.uint8)
    return np.stack([np.roll(ramp, (3 * y + seed) % w) for y in range(h)])


@pytest.mark.parametrize("search,patch", [(1, 1), (5, 2), (10, 3)])
def test_identical_rows_equal_the_argument_table(search, patch):
    from upr import denoise
    low, rect = _image("77x93 letterboxed")
    imgs = np.stack([_enhanced(low, 5), _enhanced(low[::-1], 6), _enhanced(low[:, ::-1], 7)])
    x, m = _dev(imgs), _dev(np.stack([_map(64, 64, k) for k in range(3)]))
    strengths = torch.full((3,), 2.5, dtype=torch.float64, device=DEV)
    got = denoise.nlm(x, m, None, strengths, 16, search, patch)
    want = denoise.nlm(x, m, None, 2.5, 16, search, patch)
    assert torch.equal(got, want)
    got = denoise.nlm(x[:1], m[:1], rect, strengths[:1], 16, search, patch)
    assert torch.equal(got, denoise.nlm(x[:1], m[:1], rect, 2.5, 16, search, patch))


def test_three_strengths_in_one_call():
    from upr import denoise
    low, rect = _image("77x93 letterboxed")
    imgs = np.stack([_enhanced(low, 5)] * 3)  # the same pixels: only the strength tells the images apart
    x, m = _dev(imgs), _dev(np.stack([_map(64, 64)] * 3))
    values = (0.0, 1.0, 6.0)
    got = denoise.nlm(x, m, rect, torch.tensor(values, dtype=torch.float64, device=DEV))
    outs = []
    for b, s in enumerate(values):
        one = denoise.nlm(x[b:b + 1], m[b:b + 1], rect, s)
        assert torch.equal(got[b], one[0]), f"image {b}, strength {s}"
        _assert_bytes(got[b], D.nlm(imgs[b], _map(64, 64), rect, s), f"image {b}")
        outs.append(one[0])
    _assert_bytes(got[0], imgs[0], "strength 0 is the identity")
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])


@pytest.mark.parametrize("name", ["40x56 noise", "77x93 letterboxed", "left bar 13", "3 rows", "2 rows",
                                  "128x128 constant", "extremes", "70x67 in 128x131"])
def test_nlm_auto_equals_the_restatement(name):
    from upr import denoise
    low, rect = _image(name)
    src = _enhanced(low, 8)
    m = _map(*low.shape[:2])
    for scale, search, patch in ((1.0, 3, 1), (1.7, 2, 2)):
        got = denoise.nlm_auto(_dev(src)[None], _dev(low)[None], _dev(m)[None], rect, scale, 16, search, patch)
        want = N.nlm_auto(src, low, m, rect, scale, 16, search, patch)
        _assert_bytes(got[0], want, f"{name} scale {scale}")
        if N.sigma(low, rect) == 0.0:
            _assert_bytes(got[0], src, f"{name}: sigma 0 is the identity")


def test_nlm_auto_batch_uses_each_images_own_estimate():
    from upr import denoise
    g4 = _g4()[:64, :64]
    lows = np.stack([_noised(g4 // 3 + 10, s, 30 + k) for k, s in enumerate((0.4, 2.0, 5.0))])
    srcs = np.stack([np.clip(3.0 * (a.astype(np.float64) - 10), 0, 255).astype(np.uint8) for a in lows])
    got = denoise.nlm_auto(_dev(srcs), _dev(lows), None, None, 1.0, 16, 3, 1)
    for b in range(3):
        _assert_bytes(got[b], N.nlm_auto(srcs[b], lows[b], None, None, 1.0, 16, 3, 1), f"image {b}")


# ---------------------------------------------------------------------------
# 4. refused arguments: the error code, nothing launched
# ---------------------------------------------------------------------------
def test_refused_arguments():
    from upr import _lib as L, denoise
    from upr.runtime import _ptr
    lib = L.lib()
    x = _dev(_image("40x56 noise")[0])[None]
    sig = torch.full((1,), -7.0, dtype=torch.float64, device=DEV)
    ws_bytes = lib.upr_noise_sigma_workspace(1)
    assert ws_bytes >= 2041 * 4 and lib.upr_noise_sigma_workspace(0) == 0
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=DEV)

    def sigma(src=_ptr(x), B=1, H=40, W=56, rect=(0, 0, 40, 56), out=_ptr(sig), w=_ptr(ws), nbytes=ws_bytes):
        return lib.upr_noise_sigma_u8(src, B, H, W, *rect, out, w, ctypes.c_size_t(nbytes), None)

    ARG, SHAPE, WS = -1, -2, -4
    assert sigma(src=None) == ARG and sigma(out=None) == ARG and sigma(w=None) == ARG and sigma(B=0) == ARG
    for rect in ((1, 0, 40, 56), (0, 1, 40, 56), (-1, 0, 10, 10), (0, 0, 0, 10), (0, 0, 10, 0)):
        assert sigma(rect=rect) == ARG, rect
    assert sigma(B=65536) == SHAPE
    assert sigma(H=30000, W=30000, rect=(0, 0, 27000, 27000)) == SHAPE  # 3 nh nw >= 2^31
    assert sigma(nbytes=ws_bytes - 1) == WS
    tables = torch.full((1, 256), 5, dtype=torch.int32, device=DEV)

    def lut_dev(s=_ptr(sig), B=1, scale=1.0, floor=16, patch=2, t=_ptr(tables)):
        return lib.upr_denoise_lut_dev(s, B, ctypes.c_double(scale), floor, patch, t, None)

    for kw in (dict(s=None), dict(t=None), dict(B=0), dict(scale=-1.0), dict(scale=float("inf")),
               dict(scale=float("nan")), dict(floor=0), dict(floor=256), dict(patch=0), dict(patch=4)):
        assert lut_dev(**kw) == ARG, kw
    out = torch.full_like(x, 9)

    def luts(src=_ptr(x), B=1, rect=(0, 0, 40, 56), search=5, patch=2, t=_ptr(tables), o=_ptr(out), stride=0):
        return lib.upr_denoise_nlm_u8_luts(src, None, stride, B, 40, 56, *rect, search, patch, t, o, None)

    for kw in (dict(src=None), dict(t=None), dict(o=None), dict(o=_ptr(x)), dict(B=0), dict(rect=(0, 1, 40, 56)),
               dict(search=11), dict(patch=0)):
        assert luts(**kw) == ARG, kw
    assert luts(B=65536) == SHAPE
    torch.cuda.synchronize()
    assert float(sig[0]) == -7.0 and bool((tables == 5).all()) and bool((out == 9).all())  # nothing ran
    # the Python layer
    with pytest.raises(RuntimeError):
        denoise.estimate_sigma(x.cpu())
    with pytest.raises(ValueError):
        denoise.estimate_sigma(x, (0, 0, 41, 56))
    with pytest.raises(ValueError):
        denoise.nlm(x, strength=torch.ones(2, dtype=torch.float64, device=DEV))  # two strengths, one image
    with pytest.raises(ValueError):
        denoise.nlm(x, strength=torch.ones(1, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        denoise.nlm(x, strength="auto")
    with pytest.raises(ValueError):
        denoise.nlm_auto(x, x[:, :20])
    with pytest.raises(ValueError):
        denoise.nlm_auto(x, x, scale=-1.0)


# ---------------------------------------------------------------------------
# 5. the harness
# ---------------------------------------------------------------------------
KW = dict(use_preact=False, use_aspp=False, seed=0)
AUTO = dict(denoise="nlm", denoise_strength="auto", denoise_search=3, denoise_patch=1)
REF = dict(search=3, patch=1)


@pytest.fixture(scope="module")
def pipe(tmp_path_factory):
    """The input directory (three 77 x 93 images of different noise levels that share a batch, a
    128 x 128 and a 40 x 40 one), and the files of a max_size 64 run with denoise off."""
    from enhancers.simple_enhance import enhance_batch_images
    root = tmp_path_factory.mktemp("noise")
    src = root / "in"
    src.mkdir()
    g4 = _g4()
    dark = lambda a: np.rint(a * 0.4 + 6).astype(np.uint8)  # noqa: E731
    images = {"a77": dark(g4[:77, :93]), "b77": _noised(dark(g4[51:, 35:]), 2.0, 41),
              "e77": _noised(dark(g4[:77, :93]), 6.0, 42), "c128": _noised(dark(g4), 3.0, 43),
              "d40": _noised(dark(g4[:40, :40]), 1.0, 44)}
    for k, a in images.items():
        Image.fromarray(np.ascontiguousarray(a)).save(src / f"{k}.png")
    enhance_batch_images(str(src), str(root / "off"), DEV, max_size=64, **KW)
    off = {n: {s: np.asarray(Image.open(root / "off" / f"{n}_{s}.png")) for s in SUFFIXES} for n in images}
    want, sigmas = {}, {}
    for n, a in images.items():  # the restatement on the off run's files; the input is the left panel
        rect = G.content_rect(a.shape[:2], 64)
        Wl = off[n]["enhanced"].shape[1]
        low = off[n]["comparison"][:, :Wl]
        sigmas[n] = N.sigma(low, rect)
        want[n] = N.nlm_auto(off[n]["enhanced"], low, off[n]["illumination"], rect, **REF)
        assert (want[n] != off[n]["enhanced"]).any()
    assert sigmas["a77"] < sigmas["b77"] < sigmas["e77"], sigmas  # one batch, three noise levels
    return root, src, images, off, want


def _check_letterboxed(out, images, off, want, panels=2):
    for n in images:
        Wl = want[n].shape[1]
        np.testing.assert_array_equal(np.asarray(Image.open(out / f"{n}_enhanced.png")), want[n], err_msg=n)
        np.testing.assert_array_equal(np.asarray(Image.open(out / f"{n}_illumination.png")), off[n]["illumination"])
        if panels:
            cmp = np.asarray(Image.open(out / f"{n}_comparison.png"))
            assert cmp.shape[1] == panels * Wl
            np.testing.assert_array_equal(cmp[:, Wl:2 * Wl], want[n], err_msg=f"{n} panel")
            np.testing.assert_array_equal(cmp[:, :Wl], off[n]["comparison"][:, :Wl])
            if panels == 3:
                np.testing.assert_array_equal(cmp[:, 2 * Wl:], off[n]["illumination"])


@pytest.mark.parametrize("encoder", ["host", "device"])
def test_files_equal_the_restatement_on_the_off_files(pipe, tmp_path, encoder):
    from enhancers.simple_enhance import enhance_batch_images
    root, src, images, off, want = pipe
    names = sorted(f"{n}_{s}.png" for n in images for s in SUFFIXES)
    for bs in (1, 4):
        out = tmp_path / str(bs)
        enhance_batch_images(str(src), str(out), DEV, max_size=64, batch_size=bs, png_encoder=encoder, **KW, **AUTO)
        assert sorted(os.listdir(out)) == names
        _check_letterboxed(out, images, off, want)
    for f in names:  # batch 1 and batch 4 write identical files
        assert open(tmp_path / "1" / f, "rb").read() == open(tmp_path / "4" / f, "rb").read(), f


@pytest.mark.parametrize("encoder", ["host", "device"])
def test_run_batched_with_and_without_the_comparison(pipe, tmp_path, encoder):
    from enhancers.simple_enhance import list_images, run_batched
    from models.model import UP_Retinex
    root, src, images, off, want = pipe
    torch.manual_seed(0)
    model = UP_Retinex(use_preact=False, use_aspp=False).to(DEV).eval()
    for bs in (1, 4):
        for comparison in (None, 2):
            out = tmp_path / f"{bs}_{comparison}"
            run_batched(model, list_images(str(src)), str(out), DEV, max_size=64, batch_size=bs, png_encoder=encoder,
                        comparison=comparison, image_lines=False, **AUTO)
            kinds = SUFFIXES if comparison else SUFFIXES[:2]
            assert sorted(os.listdir(out)) == sorted(f"{n}_{s}.png" for n in images for s in kinds)
            _check_letterboxed(out, images, off, want, comparison or 0)


def test_auto_scale_multiplies_the_estimate(pipe, tmp_path):
    from enhancers.simple_enhance import enhance_batch_images
    root, src, images, off, _ = pipe
    enhance_batch_images(str(src), str(tmp_path), DEV, max_size=64, batch_size=4, denoise_auto_scale=2.5, **KW, **AUTO)
    for n in ("a77", "b77", "e77"):
        low = off[n]["comparison"][:, :64]
        want = N.nlm_auto(off[n]["enhanced"], low, off[n]["illumination"], (5, 0, 53, 64), 2.5, **REF)
        np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / f"{n}_enhanced.png")), want, err_msg=n)


def test_original_size_files(pipe, tmp_path):
    from enhancers.simple_enhance import enhance_batch_images
    root, src, images, off, want = pipe
    for bs in (1, 4):
        enhance_batch_images(str(src), str(tmp_path / str(bs)), DEV, max_size=64, batch_size=bs,
                             output_size="original", **KW, **AUTO)
    names = sorted(f"{n}_{s}.png" for n in images for s in SUFFIXES)
    assert sorted(os.listdir(tmp_path / "1")) == names == sorted(os.listdir(tmp_path / "4"))
    for f in names:
        assert open(tmp_path / "1" / f, "rb").read() == open(tmp_path / "4" / f, "rb").read(), f
    top, left, nh, nw = G.content_rect((40, 40), 64)  # nothing was resized: the crop of the denoised pixels
    np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "1" / "d40_enhanced.png")),
                                  want["d40"][top:top + nh, left:left + nw])
    for n in ("a77", "e77"):  # the resized ones: the restore of the denoised target
        lb = off[n]
        ref = G.restore(np.ascontiguousarray(images[n]), lb["comparison"][:, :64], want[n], lb["illumination"],
                        G.content_rect((77, 93), 64), comparison=2)
        for s, w in zip(SUFFIXES, ref):
            np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "1" / f"{n}_{s}.png")), w, err_msg=n + s)


def test_single_image_path(pipe, tmp_path):
    from enhancers.simple_enhance import enhance_single_image, load_image
    from models.model import UP_Retinex
    from upr import runtime
    _, src, images, _, _ = pipe
    torch.manual_seed(0)
    model = UP_Retinex(use_preact=False, use_aspp=False).to(DEV).eval()
    path = str(src / "e77.png")
    enh, illu = enhance_single_image(model, path, str(tmp_path), DEV, max_size=64, **AUTO)
    x, _ = load_image(path, 64, device=DEV)
    low, tgt, ill = (runtime.to_u8_hwc(t[0]).cpu().numpy() for t in (x, enh, illu))
    want = N.nlm_auto(tgt, low, ill, (5, 0, 53, 64), **REF)
    assert (want != tgt).any()
    np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "e77_enhanced.png")), want)
    np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "e77_comparison.png")),
                                  np.concatenate([low, want], axis=1))


def test_predict_mode_with_and_without_the_comparison(pipe, tmp_path):
    import main as cli
    from models.model import UP_Retinex
    _, src, images, _, _ = pipe
    torch.manual_seed(0)
    ckpt = str(tmp_path / "m.pth")
    torch.save({"model_state_dict": UP_Retinex(use_preact=False, use_aspp=False).state_dict()}, ckpt)
    base = ["--mode", "predict", "--checkpoint", ckpt, "--input_path", str(src), "--device", DEV, "--max_size", "64"]
    cli.main(base + ["--output_dir", str(tmp_path / "off")])
    off = {n: {s: np.asarray(Image.open(tmp_path / "off" / f"{n}_{s}.png")) for s in SUFFIXES} for n in images}
    want = {n: N.nlm_auto(off[n]["enhanced"], off[n]["comparison"][:, :off[n]["enhanced"].shape[1]],
                          off[n]["illumination"], G.content_rect(a.shape[:2], 64), **REF) for n, a in images.items()}
    auto = ["--denoise", "nlm", "--denoise_strength", "auto", "--denoise_search", "3", "--denoise_patch", "1"]
    runs = (("loop", [], 3), ("batched", ["--infer_batch", "4"], 3),
            ("bare", ["--infer_batch", "4", "--no_comparison"], 0),
            ("bare_device", ["--infer_batch", "4", "--no_comparison", "--png_encoder", "device"], 0),
            ("loop_bare", ["--no_comparison"], 0))
    for tag, extra, panels in runs:
        out = tmp_path / tag
        cli.main(base + ["--output_dir", str(out)] + auto + extra)
        kinds = SUFFIXES if panels else SUFFIXES[:2]
        assert sorted(os.listdir(out)) == sorted(f"{n}_{s}.png" for n in images for s in kinds), tag
        _check_letterboxed(out, images, off, want, panels)


def test_evaluate_mode_noise_sigma_column(pipe, tmp_path):
    import main as cli
    from enhancers.simple_enhance import load_image
    from upr import runtime
    from utils.utils import batch_noise_sigma, calculate_noise_sigma, metric_names
    _, src, images, _, _ = pipe
    base = ["--mode", "evaluate", "--input_path", str(src), "--device", DEV]
    cli.main(base + ["--output_dir", str(tmp_path / "plain")])
    cli.main(base + ["--output_dir", str(tmp_path / "sigma"), "--noise_sigma"])
    cli.main(base + ["--output_dir", str(tmp_path / "both"), "--noise_sigma", "--lowlight_dir", str(src)])
    plain = open(tmp_path / "plain" / "metrics.csv").read().splitlines()
    rows = open(tmp_path / "sigma" / "metrics.csv").read().splitlines()
    assert plain[0] == ",".join(("file",) + tuple(metric_names(False)))  # unchanged without the flag
    assert rows[0] == plain[0] + ",noise_sigma"
    assert [r.rsplit(",", 1)[0] for r in rows] == plain
    assert open(tmp_path / "both" / "metrics.csv").readline().strip() == plain[0] + ",loe,noise_sigma"
    values = []
    for r, n in zip(rows[1:], sorted(images)):
        x, _ = load_image(str(src / f"{n}.png"), None, device=DEV)
        want = N.sigma(runtime.to_u8_hwc(x[0]).cpu().numpy())
        assert r.split(",")[0] == f"{n}.png" and r.rsplit(",", 1)[1] == repr(want), (n, r, want)
        assert calculate_noise_sigma(x) == want and calculate_noise_sigma(x[0].cpu().numpy()) == want
        values.append(want)
    assert rows[-1].rsplit(",", 1)[1] == repr(sum(values) / len(values))
    x = torch.cat([load_image(str(src / f"{n}.png"), None, device=DEV)[0] for n in ("a77", "e77")])
    assert batch_noise_sigma(x).cpu().tolist() == [values[0], values[4]]
