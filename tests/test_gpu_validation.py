"""Validation in `main.py --mode train` (trainers.train.validate, --val_dir and
friends) on small generated directories: the val_* columns of results.csv
against validate() itself and against a loop written here, the state validate
must leave alone, --best_by, the sample panels, and the unchanged defaults."""
import copy
import csv
import math
import random

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]
DEV = "cuda:0"
KEYS = ["total", "exposure", "smoothness", "color", "spatial", "decouple", "perceptual"]
METRICS_PAIRED = ["mean_brightness", "contrast", "entropy", "niqe", "psnr", "ssim", "mse", "saturation",
                  "naturalness"]
VAL_PAIRED = ["val_" + k for k in KEYS + METRICS_PAIRED + ["loe"]]
VAL_UNPAIRED = [c for c in VAL_PAIRED if c not in ("val_psnr", "val_ssim", "val_mse")]
STEMS = ["v0", "v1", "v2"]


class _Spy:
    """Records what train(args) hands to save_checkpoint."""

    def __init__(self, mp):
        from trainers import train as T
        self.saved, self.model = [], None
        save = T.save_checkpoint

        def spy_save(model, optimizer, epoch, save_dir, is_best=False):
            self.model = model
            self.saved.append((epoch, is_best))
            return save(model, optimizer, epoch, save_dir, is_best)

        mp.setattr(T, "save_checkpoint", spy_save)


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    root = tmp_path_factory.mktemp("val")
    rng = np.random.default_rng(9)
    for name in ("train", "val", "gt"):
        (root / name).mkdir()
    for i in range(6):
        Image.fromarray((rng.integers(0, 256, (64, 64, 3)) * 0.4).astype(np.uint8)).save(root / "train" / f"low{i}.png")
    for s in STEMS:
        gt = rng.integers(0, 256, (64, 64, 3))
        Image.fromarray(gt.astype(np.uint8)).save(root / "gt" / f"{s}.png")
        Image.fromarray((gt * 0.3).astype(np.uint8)).save(root / "val" / f"{s}.png")
    return root


def _argv(dirs, save, *extra):
    return ["--mode", "train", "--train_dir", str(dirs / "train"), "--save_dir", str(save), "--batch_size", "2",
            "--image_size", "64", "--num_workers", "2", "--seed", "0", "--device", DEV, "--num_epochs", "2",
            *extra]


def _train(dirs, save, *extra):
    import main as cli
    with pytest.MonkeyPatch.context() as mp:
        spy = _Spy(mp)
        cli.main(_argv(dirs, save, *extra))
    return spy, list(csv.DictReader(open(save / "results.csv")))


@pytest.fixture(scope="module")
def paired_run(dirs):
    """2 epochs with --val_dir and ground truth, best by the default train_total, host-encoded panels."""
    save = dirs / "ckpt_paired"
    spy, rows = _train(dirs, save, "--val_dir", str(dirs / "val"), "--val_reference_dir", str(dirs / "gt"),
                       "--val_samples", "2")
    return spy, rows, save


@pytest.fixture(scope="module")
def plain_run(dirs):
    save = dirs / "ckpt_plain"
    spy, rows = _train(dirs, save)
    return spy, rows, save


def _loaders(dirs, paired=True):
    from trainers import train as T
    return T.make_val_loaders(str(dirs / "val"), str(dirs / "gt") if paired else None, image_size=64, batch_size=2,
                              num_workers=2, device=torch.device(DEV))


def _criterion(**kw):
    from losses.loss import TotalLoss
    return TotalLoss(use_freq_loss=False, **kw).to(DEV)


def test_csv_columns_and_last_row_equal_validate(paired_run, dirs):
    from trainers import train as T
    spy, rows, _ = paired_run
    assert len(rows) == 2 and list(rows[0]) == ["epoch"] + KEYS + VAL_PAIRED
    assert T.val_columns(True) == VAL_PAIRED and T.val_columns(False) == VAL_UNPAIRED
    assert all(math.isfinite(float(r[k])) for r in rows for k in KEYS + VAL_PAIRED)
    loader, refs = _loaders(dirs)
    # the trained module the run handed to save_checkpoint: the same weights through the same forward
    got = T.validate(spy.model, loader, _criterion(), torch.device(DEV), reference_loader=refs)
    assert list(got) == VAL_PAIRED
    assert spy.model.training
    for k in VAL_PAIRED:
        assert float(rows[-1][k]) == got[k], (k, rows[-1][k], got[k])


def test_validate_arithmetic_against_a_loop_written_here(paired_run, dirs):
    from trainers import train as T
    from upr.loss_engine import TERM_ORDER
    from utils.utils import batch_loe, batch_metrics
    spy, _, _ = paired_run
    model, crit = spy.model, _criterion()
    for paired, cols in ((True, VAL_PAIRED), (False, VAL_UNPAIRED)):
        loader, refs = _loaders(dirs, paired)
        got = T.validate(model, loader, crit, torch.device(DEV), reference_loader=refs, loe_size=16)
        loader, refs = _loaders(dirs, paired)
        want, n = {c: 0.0 for c in cols}, 0
        model.eval()
        sizes = []
        with torch.no_grad():
            for low, gt in zip(loader, refs if paired else [None, None]):
                enh, refl, illu = model(low)
                terms = crit.evaluate(low, enh, illu, refl).double().cpu().tolist()
                m = batch_metrics(enh, gt)
                loe = batch_loe(low, enh, 16)
                b = low.shape[0]
                sizes.append(b)
                for k in KEYS:
                    want["val_" + k] += terms[TERM_ORDER.index(k)] * b
                for k in m:
                    want["val_" + k] += float(m[k].sum().cpu())
                want["val_loe"] += float(loe.sum().cpu())
                n += b
        model.train()
        assert sizes == [2, 1] and n == 3  # the short last batch is kept
        assert list(got) == cols
        for c in cols:
            w = want[c] / n
            assert abs(got[c] - w) <= 1e-12 * abs(w), (c, got[c], w)
        assert got["val_loe"] > 0


def _snapshot(model, opt, scaler, crit):
    snap = {"model": {k: v.detach().clone() for k, v in model.state_dict().items()},
            "opt": {k: (v.detach().clone() if torch.is_tensor(v) else copy.deepcopy(v))
                    for k, v in opt.state_dict().items()},
            "scaler": copy.deepcopy(scaler.state_dict()) if scaler is not None else None,
            "history": copy.deepcopy(crit.loss_history), "random": random.getstate()}
    return snap


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "amp"])
def test_validate_leaves_the_run_as_it_found_it(dirs, amp):
    from models.model import MultiScaleUP_Retinex
    from trainers import train as T
    torch.manual_seed(0)
    model = MultiScaleUP_Retinex(use_preact=False, use_aspp=False).to(DEV)
    crit = _criterion(adaptive_weights=True)
    opt = T.make_optimizer(model, lr=1e-4, weight_decay=1e-5)
    scaler = T.GradScaler() if amp else None
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(3)).to(DEV) * 0.4
    model.train()

    def step():
        _, d = T.train_step(model, x, crit, opt, scaler=scaler, use_amp=amp)
        return d["total"]

    step()
    step()
    before = _snapshot(model, opt, scaler, crit)
    assert len(before["history"]["exposure"]) == 2 and any("running_mean" in k for k in before["model"])
    assert any("num_batches_tracked" in k for k in before["model"])
    loader, refs = _loaders(dirs)
    val = T.validate(model, loader, crit, torch.device(DEV), reference_loader=refs)
    after = _snapshot(model, opt, scaler, crit)
    assert model.training and all(m.training for m in model.modules())
    for part in before:
        assert _same(before[part], after[part]), part
    assert all(math.isfinite(v) for v in val.values())
    # the engine's per-step state (re-packed weights, fp16 copies) survives the eval / train switch: the step
    # after validation gives the loss of the same step from the restored snapshot with no validation before it.
    # Weight-gradient sums are atomic (order differences near 1e-6), a forward on weights one step stale would
    # differ near lr = 1e-4 per weight: 1e-5 relative separates the two.
    third = step()
    model.load_state_dict(before["model"])
    opt.load_state_dict(before["opt"])
    if scaler is not None:
        scaler.load_state_dict(before["scaler"])
    crit.loss_history = copy.deepcopy(before["history"])
    again = step()
    assert abs(third - again) <= 1e-5 * abs(again), (third, again)


def test_best_by_train_total_ignores_validation(paired_run, plain_run):
    spy, rows, _ = paired_run
    spy0, rows0, save0 = plain_run
    assert [s for s in spy.saved] == [s for s in spy0.saved] and spy.saved[0] == (0, True)
    # defaults: today's header, no samples directory
    assert list(rows0[0]) == ["epoch"] + KEYS
    assert not (save0 / "samples").exists()
    # validation did not disturb the training it ran between (atomic weight-gradient sums: not bit for bit)
    for r, r0 in zip(rows, rows0):
        assert float(r["total"]) == pytest.approx(float(r0["total"]), rel=1e-3)


def _check_panels(sample_dir, dirs, stems, ext="png"):
    from upr import runtime
    files = sorted(p.name for p in sample_dir.iterdir())
    assert files == [f"{s}_comparison.{ext}" for s in stems]
    loader, _ = _loaders(dirs, paired=False)
    low = torch.cat(list(loader))
    for i, s in enumerate(stems):
        im = Image.open(sample_dir / f"{s}_comparison.{ext}")
        assert im.size == (192, 64) and im.mode == "RGB"
        left = np.asarray(im)[:, :64]
        assert np.array_equal(left, runtime.to_u8_hwc(low[i]).cpu().numpy()), s


def test_best_by_val_loe_and_device_encoded_panels(dirs):
    save = dirs / "ckpt_loe"
    spy, rows = _train(dirs, save, "--val_dir", str(dirs / "val"), "--best_by", "val_loe", "--png_encoder", "device",
                       "--lr", "0.01")
    assert list(rows[0]) == ["epoch"] + KEYS + VAL_UNPAIRED
    loe = [float(r["val_loe"]) for r in rows]
    want, best = [], float("inf")
    for v in loe:
        want.append(v < best)
        best = min(best, v)
    assert [s[1] for s in spy.saved] == want and want[0] is True
    assert (save / "best_model.pth").exists()
    # all three validation images (K = 4 > 3), after the last epoch only (--save_freq 10)
    assert sorted(p.name for p in (save / "samples").iterdir()) == ["epoch_0002"]
    _check_panels(save / "samples" / "epoch_0002", dirs, STEMS)


def test_host_encoded_panels_of_the_first_k(paired_run, dirs):
    _, _, save = paired_run
    assert sorted(p.name for p in (save / "samples").iterdir()) == ["epoch_0002"]
    _check_panels(save / "samples" / "epoch_0002", dirs, STEMS[:2])


def test_is_best_follows_val_loe_not_total(dirs, monkeypatch):
    """--val_freq 2 over 2 epochs: epoch 0 is not validated (no best, empty cells), epoch 1 is."""
    save = dirs / "ckpt_freq"
    spy, rows = _train(dirs, save, "--val_dir", str(dirs / "val"), "--best_by", "val_loe", "--val_freq", "2",
                       "--val_samples", "0")
    assert [s[1] for s in spy.saved] == [False, True]
    assert all(rows[0][c] == "" for c in VAL_UNPAIRED) and all(rows[1][c] != "" for c in VAL_UNPAIRED)
    assert float(rows[0]["total"]) > 0 and not (save / "samples").exists()
