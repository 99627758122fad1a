"""Device lightness order error (csrc/loe.hip via upr.runtime.image_loe,
utils.utils.batch_loe / calculate_loe and main.py --mode evaluate
--lowlight_dir): (D, N) equal as integers to the numpy restatement
(tests/loe_ref.py) and loe == D / N bit for bit, at the shapes where the
kernels take another path; batching, reruns, workspace reuse, fp16, input
forms and the evaluate column."""
import csv

import numpy as np
import pytest
import torch
from PIL import Image

import loe_ref as R
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(low, enh, sample):
    """numpy [3,H,W] pair -> (D, N, loe) python numbers from one device call."""
    from upr import runtime
    v, c = runtime.image_loe(_dev(low)[None], _dev(enh)[None], sample, counts=True)
    assert v.dtype == torch.float64 and v.shape == (1,) and c.dtype == torch.int64 and c.shape == (1, 2)
    D, N = c[0].cpu().tolist()
    return D, N, float(v.cpu()[0])


def _check(low, enh, sample, tag, pairs=False):
    D, N, v = _run(low, enh, sample)
    wD, wN, wv = R.loe(low, enh, sample, pairs=pairs)
    print(f"{tag}: D {D} N {N} loe {v!r}")
    assert (D, N) == (wD, wN), f"{tag}: device (D, N) = {(D, N)}, restatement {(wD, wN)}"
    assert v == wv, f"{tag}: loe {v!r} is not D / N = {wv!r}"
    return D


@pytest.mark.parametrize("H,W,sample", R.SMALL)
def test_small_shapes_match_both_forms(H, W, sample):
    """tiny; odd width (unaligned rows, no 16-byte loads); subsampled grids with rounding; a full grid."""
    x, e = R.pair(H, W, seed=3)
    D = _check(x, e, sample, f"{H}x{W}/{sample}", pairs=True)
    assert D > 0


def test_int64_count_of_a_reversed_image():
    """216 x 216 at full resolution with enh = 1 - low: D > 2^31 (the histogram form is the witness)."""
    rng = np.random.default_rng(7)
    k = rng.integers(0, 256, (216, 216))
    low = np.repeat((k.astype(np.float32) / np.float32(255))[None], 3, axis=0)
    enh = np.repeat(((255 - k).astype(np.float32) / np.float32(255))[None], 3, axis=0)
    D = _check(low, enh, 0, "216x216 reversed")
    assert D > 2 ** 31


def test_one_bin_past_any_16_bit_counter():
    """260 x 260 constant images: 67 600 pixels in one bin."""
    low = np.full((3, 260, 260), 0.2, np.float32)
    enh = np.full((3, 260, 260), 0.6, np.float32)
    assert _check(low, enh, 0, "260x260 flat") == 0


def test_one_full_histogram_row():
    low = np.full((3, 260, 260), 0.2, np.float32)
    enh = np.random.default_rng(8).random((3, 260, 260), dtype=np.float32)
    _check(low, enh, 0, "260x260 constant low")
    _check(enh, low, 0, "260x260 constant enh")


def test_unaligned_full_grid_beyond_one_block():
    """131 x 131 = 17 161 pixels: odd plane size (the pixel-by-pixel reads) in the block-private form, two blocks."""
    x, e = R.pair(131, 131, seed=9)
    _check(x, e, 0, "131x131/0")
    _check(x, e, 50, "131x131/50")


def test_fp16_equals_fp32_of_the_widened_tensor():
    from upr import runtime
    for (H, W, s) in ((37, 53, 50), (136, 136, 0), (64, 96, 50)):
        x, e = R.pair(H, W, seed=10)
        x16, e16 = _dev(np.stack([x, e])).half(), _dev(np.stack([e, x])).half()
        a = runtime.image_loe(x16, e16, s, counts=True)
        b = runtime.image_loe(x16.float(), e16.float(), s, counts=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (H, W, s)
        wD, wN, wv = R.loe(x16[0].float().cpu().numpy(), e16[0].float().cpu().numpy(), s)
        assert a[1][0].cpu().tolist() == [wD, wN] and float(a[0][0].cpu()) == wv


def test_batch_equals_single_images_and_reruns_are_bit_identical():
    from upr import runtime
    from utils.utils import batch_loe
    ps = [R.pair(140, 132, seed=20 + i) for i in range(5)]
    x, e = _dev(np.stack([p[0] for p in ps])), _dev(np.stack([p[1] for p in ps]))
    for s in (50, 0):
        v, c = runtime.image_loe(x, e, s, counts=True)
        assert len({tuple(r) for r in c.cpu().tolist()}) == 5  # five different images
        for i in (4, 0, 2, 1, 3):
            vi, ci = runtime.image_loe(x[i:i + 1], e[i:i + 1], s, counts=True)
            assert torch.equal(vi[0], v[i]) and torch.equal(ci[0], c[i]), (s, i)
        for _ in range(3):
            v2, c2 = runtime.image_loe(x, e, s, counts=True)
            assert torch.equal(v2, v) and torch.equal(c2, c)
        b = batch_loe(x, e, s)
        assert b.dtype == torch.float64 and b.shape == (5,) and b.is_cuda and torch.equal(b, v)


def test_two_pairs_back_to_back_through_one_workspace():
    """The op zeroes its own workspace: the second call's table holds nothing of the first's."""
    from upr import runtime
    a, b = R.pair(150, 120, seed=30), R.pair(150, 120, seed=31)
    for s in (0, 50):
        ra = runtime.image_loe(_dev(a[0])[None], _dev(a[1])[None], s, counts=True)
        rb = runtime.image_loe(_dev(b[0])[None], _dev(b[1])[None], s, counts=True)
        torch.cuda.synchronize()
        assert ra[1][0].cpu().tolist() == list(R.loe(a[0], a[1], s)[:2])
        assert rb[1][0].cpu().tolist() == list(R.loe(b[0], b[1], s)[:2])


def test_calculate_loe_input_forms():
    from utils.utils import calculate_loe
    x, e = R.pair(37, 53, seed=11)
    want = R.loe(x, e, 50)[2]
    got = calculate_loe(_dev(x), _dev(e))
    assert isinstance(got, float) and got == want
    assert calculate_loe(x.transpose(1, 2, 0), e.transpose(1, 2, 0)) == want  # the reference's [H,W,3] host arrays
    assert calculate_loe(_dev(x)[None], _dev(e)[None], size=0) == R.loe(x, e, 0)[2]


def test_cpu_tensor_raises():
    from upr import runtime
    from utils.utils import batch_loe
    x = torch.rand(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="ROCm"):
        runtime.image_loe(x, x.to(DEV))
    with pytest.raises(RuntimeError, match="ROCm"):
        batch_loe(x.to(DEV), x)
    with pytest.raises(RuntimeError, match="match"):
        runtime.image_loe(x.to(DEV), torch.rand(1, 3, 16, 20, device=DEV))


def _write_png(path, chw):
    Image.fromarray((np.clip(chw, 0, 1) * 255).astype(np.uint8).transpose(1, 2, 0)).save(path)


def test_evaluate_mode_lowlight_dir(tmp_path):
    import main as cli
    from enhancers.simple_enhance import load_image
    from utils.utils import calculate_loe
    out_dir, low_dir, res = tmp_path / "out", tmp_path / "low", tmp_path / "res"
    out_dir.mkdir()
    low_dir.mkdir()
    names = [("a_enhanced.png", "a.png"), ("b.png", "b.png"), ("c_enhanced.png", "c.png")]
    for i, (out_name, low_name) in enumerate(names):
        x, e = R.pair(40, 56, seed=40 + i)
        _write_png(low_dir / low_name, x)
        _write_png(out_dir / out_name, e)
    argv = ["--mode", "evaluate", "--input_path", str(out_dir), "--output_dir", str(res), "--device", DEV]
    cli.main(argv + ["--lowlight_dir", str(low_dir)])
    rows = list(csv.reader(open(res / "metrics.csv")))
    assert rows[0][0] == "file" and rows[0][-1] == "loe" and "loe" not in rows[0][:-1]
    assert [r[0] for r in rows[1:]] == sorted(n[0] for n in names) + ["mean"]
    vals = []
    for (out_name, low_name), row in zip(sorted(names), rows[1:]):
        e = load_image(str(out_dir / out_name), None, device=DEV)[0]
        x = load_image(str(low_dir / low_name), None, device=DEV)[0]
        want = calculate_loe(x, e)
        assert row[-1] == repr(want) and want > 0, (out_name, row[-1], want)
        vals.append(want)
    assert float(rows[-1][-1]) == sum(vals) / 3
    before = rows
    # --loe_size reaches the op
    cli.main(argv + ["--lowlight_dir", str(low_dir), "--loe_size", "0", "--output_dir", str(res / "full")])
    full = list(csv.reader(open(res / "full" / "metrics.csv")))
    e = load_image(str(out_dir / "b.png"), None, device=DEV)[0]
    x = load_image(str(low_dir / "b.png"), None, device=DEV)[0]
    assert full[2][-1] == repr(calculate_loe(x, e, size=0)) and full[2][:-1] == before[2][:-1]
    # without the flag: no loe column, the other columns unchanged
    cli.main(argv + ["--output_dir", str(res / "plain")])
    plain = list(csv.reader(open(res / "plain" / "metrics.csv")))
    assert "loe" not in plain[0] and plain == [r[:-1] for r in before]
    # a low-light image of another size names both paths
    _write_png(low_dir / "c.png", R.pair(40, 60, seed=50)[0])
    with pytest.raises(ValueError, match=r"c\.png.*c_enhanced\.png|c_enhanced\.png.*c\.png"):
        cli.main(argv + ["--lowlight_dir", str(low_dir)])
