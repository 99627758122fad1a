"""Device image metrics (csrc/metrics.hip via upr.runtime.image_metrics,
utils.utils and main.py --mode evaluate): raw sums and histogram against the
float64 numpy restatement, calculate_metrics against the reference's recorded
outputs, batching, reruns, fp16, borders, and the evaluate mode end to end."""
import csv
import math

import numpy as np
import pytest
import torch
from PIL import Image

import metrics_ref as R
from conftest import GOLDEN, has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]
DEV = "cuda:0"
CASES = R.load_fixture(GOLDEN)
# 16 x 32 tiles: four tile rows and four tile columns, the last of each ragged (5 rows, 9 columns)
BIG = (53, 105)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(x, gt=None):
    """x, gt numpy [3,H,W] -> (metrics [9], sums [14], hist [256]) as numpy, from one device call."""
    from upr import runtime
    m, s, h = runtime.image_metrics(_dev(x)[None], None if gt is None else _dev(gt)[None], sums=True, hist=True)
    return m[0].cpu().numpy(), s[0].cpu().numpy(), h[0].cpu().numpy()


def _check_against_restatement(x, gt, tag):
    m, s, h = _run(x, gt)
    wm, ws, wh = R.metrics(x, gt)
    assert np.array_equal(h, wh), f"{tag}: histogram differs in {int((h != wh).sum())} bins"
    n = R.NSUMS if gt is not None else 10
    d = np.abs(s[:n] - ws[:n]) / np.abs(ws[:n])
    print(f"{tag}: sums worst relative difference {d.max():.2e}")
    assert (d <= 1e-10).all(), f"{tag}: sums {np.nonzero(d > 1e-10)[0].tolist()} off by {d.max():.2e}"
    if gt is None:
        assert np.isnan(s[10:]).all() and np.isnan(m[6:]).all(), f"{tag}: paired slots must be NaN without ref"
    k = len(R.NAMES) if gt is not None else 6
    dm = np.abs(m[:k] - wm[:k]) / np.abs(wm[:k])
    assert (dm <= 1e-10).all(), f"{tag}: metrics off by {dm.max():.2e}"


def test_sums_and_hist_match_restatement():
    """hist exactly; sums to 1e-10 relative (fp64 sums in another order land near 1e-13)."""
    for c in CASES:
        tag = f"{c['shape']} {c['kind']}"
        _check_against_restatement(c["x"], c["gt"], tag + " paired")
        _check_against_restatement(c["x"], None, tag + " unpaired")


def test_many_tiles_ragged_edges_match_restatement():
    rng = np.random.default_rng(11)
    gt = rng.random((3,) + BIG, dtype=np.float32)
    x = np.clip(gt + np.float32(0.2) * (rng.random((3,) + BIG, dtype=np.float32) - np.float32(0.5)), 0, 1)
    _check_against_restatement(x.astype(np.float32), gt, f"{BIG} paired")
    _check_against_restatement(x.astype(np.float32), None, f"{BIG} unpaired")


def test_calculate_metrics_matches_reference_goldens():
    """The public dict against the reference's own outputs: keys and order, 2e-6
    relative for what the reference accumulates in float32, 1e-10 for ssim and entropy."""
    from utils.utils import calculate_metrics
    bad = []
    for c in CASES:
        for paired in (False, True):
            want = c["paired" if paired else "unpaired"]
            got = calculate_metrics(_dev(c["x"])[None] if paired else _dev(c["x"]), _dev(c["gt"]) if paired else None)
            assert list(got) == list(want), (list(got), list(want))
            assert all(isinstance(v, float) for v in got.values())
            for n in want:
                d = R.rel(got[n], want[n])
                if not d <= R.tolerance(n):
                    bad.append(f"{c['shape']} {c['kind']} paired={paired} {n}: {got[n]!r} vs {want[n]!r} ({d:.2e})")
    assert not bad, "\n".join(bad)


def test_single_metric_functions_and_numpy_input():
    from utils import utils as U
    c = CASES[4]  # 13 x 70 enh
    x, gt = _dev(c["x"]), _dev(c["gt"])
    full = U.calculate_metrics(x, gt)
    assert U.calculate_psnr(x, gt) == full["psnr"] and U.calculate_ssim(x, gt) == full["ssim"]
    assert U.calculate_niqe(x) == full["niqe"] and U.calculate_saturation(x) == full["saturation"]
    assert U.calculate_naturalness(x) == full["naturalness"]
    # the reference's [H,W,C] host arrays are uploaded
    hwc = U.calculate_metrics(c["x"].transpose(1, 2, 0), c["gt"].transpose(1, 2, 0))
    assert hwc == full


def test_batch_equals_single_images_and_reruns_are_bit_identical():
    from upr import runtime
    from utils.utils import batch_metrics
    rng = np.random.default_rng(5)
    x = _dev(rng.random((5, 3, 37, 53), dtype=np.float32))
    y = _dev(rng.random((5, 3, 37, 53), dtype=np.float32))
    m, s, h = runtime.image_metrics(x, y, sums=True, hist=True)
    for i in (4, 0, 2, 1, 3):
        mi, si, hi = runtime.image_metrics(x[i:i + 1], y[i:i + 1], sums=True, hist=True)
        assert torch.equal(mi[0], m[i]) and torch.equal(si[0], s[i]) and torch.equal(hi[0], h[i]), i
    for _ in range(3):
        m2, s2, h2 = runtime.image_metrics(x, y, sums=True, hist=True)
        assert torch.equal(m2, m) and torch.equal(s2, s) and torch.equal(h2, h)
    d = batch_metrics(x, y)
    assert list(d) == list(R.PAIRED)
    for n in R.PAIRED:
        assert d[n].shape == (5,) and d[n].dtype == torch.float64 and d[n].is_cuda
        assert torch.equal(d[n], m[:, R.NAMES.index(n)])
    assert list(batch_metrics(x)) == list(R.UNPAIRED)


def test_fp16_equals_fp32_of_the_widened_tensor():
    from upr import runtime
    rng = np.random.default_rng(6)
    x16 = _dev(rng.random((2, 3, 21, 45), dtype=np.float32)).half()
    y16 = _dev(rng.random((2, 3, 21, 45), dtype=np.float32)).half()
    a = runtime.image_metrics(x16, y16, sums=True, hist=True)
    b = runtime.image_metrics(x16.float(), y16.float(), sums=True, hist=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    a = runtime.image_metrics(x16, sums=True, hist=True)
    b = runtime.image_metrics(x16.float(), sums=True, hist=True)
    assert torch.equal(a[0][:, :6], b[0][:, :6]) and torch.equal(a[1][:, :10], b[1][:, :10])
    assert torch.equal(a[2], b[2]) and torch.isnan(a[0][:, 6:]).all() and torch.isnan(a[1][:, 10:]).all()


def test_unpaired_has_no_paired_keys():
    from utils.utils import calculate_metrics
    got = calculate_metrics(_dev(CASES[3]["x"]))
    assert list(got) == list(R.UNPAIRED)
    m, s, _ = _run(CASES[3]["x"])
    assert np.isnan(m[6:]).all() and np.isfinite(m[:6]).all() and np.isnan(s[10:]).all()


def test_identical_reference_gives_psnr_100_and_ssim_1():
    from utils.utils import calculate_metrics
    for c in (CASES[0], CASES[7], CASES[12]):
        x = _dev(c["x"])
        got = calculate_metrics(x, x.clone())
        assert got["psnr"] == 100.0 and got["mse"] == 0.0
        assert abs(got["ssim"] - 1.0) <= 1e-12, got["ssim"]


def test_non_contiguous_input():
    from upr import runtime
    c = CASES[7]  # 37 x 53
    hwc = _dev(c["x"].transpose(1, 2, 0))           # [H,W,3] storage
    x = hwc.permute(2, 0, 1)[None]                  # a [1,3,H,W] view of it
    g = _dev(c["gt"])[None]
    assert not x.is_contiguous()
    a = runtime.image_metrics(x, g, sums=True, hist=True)
    b = runtime.image_metrics(x.contiguous(), g, sums=True, hist=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    wide = _dev(np.concatenate([c["x"], c["x"]], axis=2))[None]
    half = wide[..., :53]
    assert not half.is_contiguous()
    assert torch.equal(runtime.image_metrics(half, g)[0], b[0])


def test_out_of_range_values_leave_the_histogram_only():
    x = CASES[7]["x"].copy()
    x[0, 3, 4] = -0.25
    x[1, 20, 50] = 1.5
    x[2, 36, 52] = 1.0
    x[2, 0, 0] = 0.0
    m, s, h = _run(x)
    wm, ws, wh = R.metrics(x)
    assert h.sum() == x.size - 2 and np.array_equal(h, wh)
    assert np.abs(s[:10] - ws[:10]).max() <= 1e-10 * np.abs(ws[:10]).max()
    assert R.rel(s[0], float(x[0].astype(np.float64).sum())) <= 1e-12  # -0.25 is in the sums


def _write_png(path, chw):
    Image.fromarray((np.clip(chw, 0, 1) * 255).astype(np.uint8).transpose(1, 2, 0)).save(path)


def test_evaluate_mode_end_to_end(tmp_path):
    import main as cli
    from enhancers.simple_enhance import load_image
    rng = np.random.default_rng(9)
    out_dir, ref_dir, res = tmp_path / "out", tmp_path / "gt", tmp_path / "res"
    out_dir.mkdir()
    ref_dir.mkdir()
    # two sizes; references under both naming rules (same stem, and the stem without `_enhanced`)
    names = [("a.png", "a.png", (64, 96)), ("b_enhanced.png", "b.png", (64, 96)),
             ("c_enhanced.png", "c_enhanced.png", (96, 64)), ("d_enhanced.png", "d.png", (96, 64))]
    for out_name, ref_name, (h, w) in names:
        gt = rng.random((3, h, w))
        _write_png(ref_dir / ref_name, gt)
        _write_png(out_dir / out_name, gt + 0.1 * (rng.random((3, h, w)) - 0.5))
    argv = ["--mode", "evaluate", "--input_path", str(out_dir), "--reference_dir", str(ref_dir), "--output_dir",
            str(res), "--batch_size", "3", "--device", DEV]
    cli.main(argv)
    rows = list(csv.reader(open(res / "metrics.csv")))
    assert rows[0] == ["file"] + list(R.PAIRED)
    assert [r[0] for r in rows[1:]] == sorted(n[0] for n in names) + ["mean"]
    table = []
    for (out_name, ref_name, _), row in zip(sorted(names), rows[1:]):
        x = load_image(str(out_dir / out_name), None, device=DEV)[0][0].cpu().numpy()
        g = load_image(str(ref_dir / ref_name), None, device=DEV)[0][0].cpu().numpy()
        want = R.metrics_dict(x, g)
        vals = [float(v) for v in row[1:]]
        assert all(repr(v) == s for v, s in zip(vals, row[1:]))
        for n, v in zip(R.PAIRED, vals):
            assert R.rel(v, want[n]) <= R.tolerance(n), (out_name, n, v, want[n])
        table.append([want[n] for n in R.PAIRED])
    means = np.mean(np.array(table), axis=0)
    for n, v, w in zip(R.PAIRED, rows[-1][1:], means):
        assert R.rel(float(v), w) <= R.tolerance(n), ("mean", n, v, w)
    # without references: the six unpaired columns
    cli.main(["--mode", "evaluate", "--input_path", str(out_dir / "a.png"), "--output_dir", str(res / "u"),
              "--device", DEV])
    rows = list(csv.reader(open(res / "u" / "metrics.csv")))
    assert rows[0] == ["file"] + list(R.UNPAIRED) and len(rows) == 3 and rows[1][1:] == rows[2][1:]
    # a missing reference names the file
    (ref_dir / "d.png").unlink()
    with pytest.raises(ValueError, match="d_enhanced"):
        cli.main(argv)
    # a reference of another size names it too
    _write_png(ref_dir / "d.png", rng.random((3, 64, 96)))
    with pytest.raises(ValueError, match="d.png"):
        cli.main(argv)
    assert not any(math.isnan(float(v)) for v in rows[1][1:])
