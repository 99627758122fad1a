"""`main.py --mode train` end to end on a small generated directory: checkpoint
files, results.csv, the lr schedule, --resume, --use_amp, and the saved
model_state_dict in a fresh model and in the oracle."""
import csv
import math

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]
DEV = "cuda:0"
KEYS = ["total", "exposure", "smoothness", "color", "spatial", "decouple", "perceptual"]


class _Spy:
    """Records what train(args) hands to save_checkpoint / gets from load_checkpoint."""

    def __init__(self, monkeypatch):
        from trainers import train as T
        self.saved, self.loaded_step, self.model = [], None, None
        save, load = T.save_checkpoint, T.load_checkpoint

        def spy_save(model, optimizer, epoch, save_dir, is_best=False):
            self.model = model
            self.saved.append((epoch, optimizer.param_groups[0]["lr"], optimizer.step_count, is_best))
            return save(model, optimizer, epoch, save_dir, is_best)

        def spy_load(model, optimizer, path, **kw):
            r = load(model, optimizer, path, **kw)
            self.loaded_step = optimizer.step_count
            return r

        monkeypatch.setattr(T, "save_checkpoint", spy_save)
        monkeypatch.setattr(T, "load_checkpoint", spy_load)


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "amp"])
def test_main_train_resume_and_checkpoint(tmp_path, monkeypatch, amp):
    import main as cli
    from models.model import MultiScaleUP_Retinex
    from oracle import net as onet
    data, save = tmp_path / "train", tmp_path / "ckpt"
    data.mkdir()
    rng = np.random.default_rng(9)
    for i in range(6):
        Image.fromarray((rng.integers(0, 256, (64, 64, 3)) * 0.4).astype(np.uint8)).save(data / f"low{i}.png")
    argv = ["--mode", "train", "--train_dir", str(data), "--save_dir", str(save), "--batch_size", "2",
            "--image_size", "64", "--lr_decay_step", "1", "--num_workers", "2", "--seed", "0", "--device", DEV,
            "--advanced_augment"] + (["--use_amp"] if amp else [])
    spy = _Spy(monkeypatch)
    cli.main(argv + ["--num_epochs", "2"])
    assert (save / "latest_model.pth").exists() and (save / "best_model.pth").exists()
    rows = list(csv.DictReader(open(save / "results.csv")))
    assert len(rows) == 2 and list(rows[0]) == ["epoch"] + KEYS
    assert all(math.isfinite(float(r[k])) for r in rows for k in KEYS)
    # StepLR(step 1, gamma 0.5): halved after epoch 0, again after epoch 1
    assert [s[0] for s in spy.saved] == [0, 1]
    assert [s[1] for s in spy.saved] == [pytest.approx(5e-5, rel=1e-12), pytest.approx(2.5e-5, rel=1e-12)]
    assert spy.saved[0][3] is True  # the first epoch is always the best so far
    step2 = spy.saved[1][2]
    assert step2 == 6 if not amp else 0 < step2 <= 6  # 2 epochs x 3 batches (AMP may skip overflowed steps)
    ck = torch.load(save / "latest_model.pth", map_location="cpu", weights_only=True)
    assert sorted(ck) == ["epoch", "model_state_dict", "optimizer_state_dict"] and ck["epoch"] == 1
    assert ck["optimizer_state_dict"]["step"] == step2

    # the saved state in a fresh model: the trained module's eval forward (same state, same kernels)
    x = (torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(4)) * 0.5)
    fresh = MultiScaleUP_Retinex(use_preact=False, use_aspp=False)
    fresh.load_state_dict(ck["model_state_dict"])
    fresh = fresh.to(DEV).eval()
    trained = spy.model.eval()
    with torch.no_grad():
        a, b = fresh(x.to(DEV)), trained(x.to(DEV))
        ref = onet.forward(ck["model_state_dict"], x, False, False)
    for name, u, v, r in zip(("enhanced", "reflectance", "illumination"), a, b, ref):
        assert (u - v).abs().max().item() <= 1e-6, name
        assert (u.float().cpu() - r).abs().max().item() <= 1e-3, name  # the reference's naming, oracle forward

    # resume: exactly one more epoch, Adam's step count restored, the schedule continues in phase
    spy2 = _Spy(monkeypatch)
    cli.main(argv + ["--num_epochs", "3", "--resume", str(save / "latest_model.pth")])
    assert spy2.loaded_step == step2
    assert [s[0] for s in spy2.saved] == [2]
    assert spy2.saved[0][1] == pytest.approx(1.25e-5, rel=1e-12)
    assert spy2.saved[0][2] == step2 + 3 if not amp else step2 <= spy2.saved[0][2] <= step2 + 3
    assert len(list(csv.DictReader(open(save / "results.csv")))) == 1  # the epochs this call ran
    assert torch.load(save / "latest_model.pth", map_location="cpu", weights_only=True)["epoch"] == 2
