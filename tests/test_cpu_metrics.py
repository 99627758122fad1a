"""Image metrics without a device: the numpy restatement (tests/metrics_ref.py)
against the reference's recorded calculate_metrics outputs, the histogram rule
against np.histogram, the utils.utils surface, and the argument checks of the
new ABI entries (which return before any device call)."""
import ctypes

import numpy as np
import pytest
import torch

import metrics_ref as R
from conftest import GOLDEN
from upr import _lib as L


@pytest.fixture(scope="module")
def cases():
    return R.load_fixture(GOLDEN)


def test_restatement_matches_reference_goldens(cases):
    """2e-6 relative for what the reference accumulates in float32 (about 6x the
    worst difference measured when the goldens were made), 1e-10 for ssim
    (float64 in the reference) and entropy (integer counts)."""
    assert len(cases) == len(R.SHAPES) * len(R.KINDS)
    bad = []
    for c in cases:
        for paired in (False, True):
            want = c["paired" if paired else "unpaired"]
            got = R.metrics_dict(c["x"], c["gt"] if paired else None)
            assert tuple(got) == tuple(want)
            for n in want:
                d = R.rel(got[n], want[n])
                if not d <= R.tolerance(n):
                    bad.append(f"{c['shape']} {c['kind']} paired={paired} {n}: {got[n]!r} vs {want[n]!r} ({d:.2e})")
    assert not bad, "\n".join(bad)


def test_histogram_rule_matches_numpy():
    rng = np.random.default_rng(7)
    one = np.float32(1)
    edges = (np.arange(257, dtype=np.float32) / np.float32(256)).astype(np.float32)
    v = np.concatenate([
        rng.random(200000, dtype=np.float32),
        edges, np.nextafter(edges, np.float32(-1)), np.nextafter(edges, np.float32(2)),
        (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32),
        np.array([1.0, 0.0, -0.0, -1e-7, 1.0000001, -3.0, 7.5, np.nextafter(one, np.float32(2))], np.float32),
    ]).astype(np.float32)
    want, _ = np.histogram(v, bins=256, range=(0, 1))
    assert np.array_equal(R.hist_rule(v), want)
    # NaN: np.histogram refuses a range check on NaN input in some versions; the rule drops it
    assert R.hist_rule(np.array([np.nan, 0.5], np.float32)).sum() == 1


def test_restatement_borders_and_identity():
    """ref == enh: mse 0, psnr exactly 100.0, ssim 1 to rounding; the paired slots are NaN without a ground truth."""
    x = np.random.default_rng(3).random((3, 9, 12), dtype=np.float32)
    m, s, h = R.metrics(x, x)
    d = dict(zip(R.NAMES, m))
    assert d["mse"] == 0.0 and d["psnr"] == 100.0 and abs(d["ssim"] - 1.0) <= 1e-12
    m0, s0, _ = R.metrics(x)
    assert np.isnan(m0[6:]).all() and np.isnan(s0[10:]).all() and np.array_equal(m0[:6], m[:6])
    assert h.sum() == x.size


def test_utils_surface_and_count_parameters():
    from utils import utils as U
    from models.model import UP_Retinex
    for name in ("calculate_metrics", "calculate_psnr", "calculate_ssim", "calculate_niqe", "calculate_saturation",
                 "calculate_naturalness", "count_parameters", "print_model_summary", "ensure_dir", "batch_metrics"):
        assert callable(getattr(U, name)), name
    model = UP_Retinex()
    total, trainable = U.count_parameters(model)
    assert total == sum(p.numel() for p in model.parameters()) > 0
    assert trainable == sum(p.numel() for p in model.parameters() if p.requires_grad)
    assert U.metric_names(False) == R.UNPAIRED and U.metric_names(True) == R.PAIRED
    assert L.METRIC_NAMES == R.NAMES and L.UPR_METRICS_NSUMS == R.NSUMS and L.UPR_METRICS_N == len(R.NAMES)


def test_metrics_refuse_cpu_tensors():
    if torch.cuda.is_available():
        pytest.skip("a ROCm device is present")
    from utils import utils as U
    from upr import runtime
    x = torch.rand(3, 8, 8)
    for call in (lambda: U.calculate_metrics(x), lambda: U.calculate_psnr(x, x), lambda: U.batch_metrics(x[None]),
                 lambda: runtime.image_metrics(x[None]), lambda: U.calculate_niqe(x.numpy().transpose(1, 2, 0))):
        with pytest.raises(RuntimeError, match="ROCm"):
            call()


def test_abi_rejects_bad_arguments_before_any_device_call():
    lib = L.lib()
    assert lib.upr_image_metrics_workspace(0, 8, 8) == 0
    need = lib.upr_image_metrics_workspace(2, 40, 70)
    assert need >= 2 * 256 * 4 + 2 * R.NSUMS * 8
    assert lib.upr_image_metrics_workspace(4, 40, 70) > need  # grows with the batch
    # never dereferenced: every call below returns from the argument checks
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    big = ctypes.c_size_t(1 << 30)

    def call(enh=p, ref=None, metrics=p, ws=p, nbytes=big, B=2, H=40, W=70, dtype=L.UPR_F32):
        return lib.upr_image_metrics(enh, ref, metrics, None, None, ws, nbytes, B, H, W, dtype, None)

    assert call(enh=None) == L.UPR_ERR_ARG
    assert call(metrics=None) == L.UPR_ERR_ARG
    assert call(ws=None) == L.UPR_ERR_ARG
    assert call(dtype=7) == L.UPR_ERR_ARG
    assert call(H=7) == L.UPR_ERR_SHAPE
    assert call(W=7) == L.UPR_ERR_SHAPE
    assert call(B=0) == L.UPR_ERR_SHAPE
    assert call(nbytes=ctypes.c_size_t(need - 1)) == L.UPR_ERR_WORKSPACE
    assert call(nbytes=ctypes.c_size_t(0)) == L.UPR_ERR_WORKSPACE


def test_parser_accepts_evaluate_mode():
    import main as cli
    a = cli.build_parser().parse_args(["--mode", "evaluate", "--input_path", "out", "--reference_dir", "gt",
                                       "--batch_size", "4", "--max_size", "256"])
    assert a.mode == "evaluate" and a.reference_dir == "gt" and a.batch_size == 4 and a.max_size == 256
    assert cli.build_parser().parse_args([]).reference_dir is None


def test_reference_lookup_rules(tmp_path):
    import main as cli
    from PIL import Image
    for n in ("a.png", "b.jpg"):
        Image.new("RGB", (8, 8)).save(tmp_path / n)
    assert cli._reference_for("x/a.png", str(tmp_path)).endswith("a.png")
    assert cli._reference_for("x/b_enhanced.png", str(tmp_path)).endswith("b.jpg")
    with pytest.raises(ValueError, match="c_enhanced"):
        cli._reference_for("x/c_enhanced.png", str(tmp_path))
