"""Paired training through the loss engine, the step and the CLI (run with `-m
gpu`), at 2x3x64x64: TotalLoss with a target against the same call without one
and the op's own output (upr.loss_engine.paired_terms), the same under the AMP
scaler, ten train_step calls on one fixed pair, and `main.py --mode train
--train_reference_dir` on four generated 48 x 40 PNG pairs."""
import csv
import math

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import has_gpu
from op_parity import _within_ulp

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]
DEV = "cuda:0"
KEYS = ["total", "exposure", "smoothness", "color", "spatial", "decouple", "perceptual"]
UNPAIRED = ("exposure", "smoothness", "color", "spatial", "decouple", "perceptual", "frequency", "smooth_weight")
W_REC, W_SSIM = 0.8, 1.7


def _inputs(seed=0, H=64, W=64):
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(2, 3, H, W, generator=g) * 0.4
    enh = torch.rand(2, 3, H, W, generator=g)
    illu = torch.rand(2, 1, H, W, generator=g) * 0.8 + 0.1
    refl = enh / (illu + 1e-6)
    target = (0.8 * enh + 0.2 * torch.rand(2, 3, H, W, generator=g)).clamp(0, 1)
    return [t.to(DEV) for t in (low, enh, illu, refl, target)]


def _run(crit, low, enh, illu, refl, target, scaler=None):
    """One forward + backward -> (loss_dict, total as a float32 numpy scalar, enh.grad, illu.grad, refl.grad)."""
    e, i, r = (t.clone().requires_grad_(True) for t in (enh, illu, refl))
    with torch.autocast("cuda", dtype=torch.float16, enabled=scaler is not None):
        total, d = crit(low, e, i, r) if target is None else crit(low, e, i, r, target=target)
    (total if scaler is None else scaler.scale(total)).backward()
    torch.cuda.synchronize()
    return dict(d.items()), total.detach().cpu().numpy(), e.grad.cpu(), i.grad.cpu(), r.grad.cpu()


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "amp"])
def test_total_loss_with_a_target(amp):
    from losses.loss import TotalLoss
    from upr import amp as uamp
    from upr.loss_engine import paired_terms
    low, enh, illu, refl, target = _inputs()
    crit = TotalLoss(weight_rec=W_REC, weight_ssim=W_SSIM).to(DEV)
    scaler = uamp.GradScaler() if amp else None
    scale = scaler.get_scale() if amp else 1.0
    d0, t0, ge0, gi0, gr0 = _run(crit, low, enh, illu, refl, None, scaler)
    d1, t1, ge1, gi1, gr1 = _run(crit, low, enh, illu, refl, target, scaler)
    assert list(d1) == list(d0) + ["reconstruction", "ssim_loss"]
    for k in UNPAIRED:
        assert np.float32(d1[k]).tobytes() == np.float32(d0[k]).tobytes(), k
    # the op on its own: its scalars, and its gradient into a zeroed buffer
    g = torch.zeros_like(enh)
    out2 = paired_terms(enh, target, crit.rec_eps, W_REC, W_SSIM, g_enh=g).cpu().numpy()
    assert (np.float32(d1["reconstruction"]), np.float32(d1["ssim_loss"])) == (out2[0], out2[1])
    assert d1["reconstruction"] > 0 and 0 < d1["ssim_loss"] < 1
    add = float(np.float32(W_REC)) * float(out2[0]) + float(np.float32(W_SSIM)) * float(out2[1])
    _within_ulp("total with a target", torch.tensor([float(t1)]), [float(t0) + add], ulps=2.0)
    assert np.float32(d1["total"]) == t1
    _within_ulp("enh.grad with a target", ge1 / scale, (ge0.double() / scale + g.cpu().double()).numpy(), ulps=2.0)
    assert torch.equal(gi1, gi0) and torch.equal(gr1, gr0)
    assert g.abs().max().item() > 0

    # a target with both weights 0 changes only the two added keys
    zero = TotalLoss().to(DEV)
    z0 = _run(zero, low, enh, illu, refl, None, scaler)
    z1 = _run(zero, low, enh, illu, refl, target, scaler)
    assert {k: v for k, v in z1[0].items() if k not in ("reconstruction", "ssim_loss")} == z0[0]
    assert (np.float32(z1[0]["reconstruction"]), np.float32(z1[0]["ssim_loss"])) == (out2[0], out2[1])
    assert z1[1] == z0[1] and all(torch.equal(a, b) for a, b in zip(z1[2:], z0[2:]))


def test_target_that_requires_grad_is_refused():
    from losses.loss import TotalLoss
    low, enh, illu, refl, target = _inputs()
    crit = TotalLoss(weight_rec=1.0, weight_perceptual=0.0).to(DEV)
    with pytest.raises(NotImplementedError, match="target"):
        crit(low, enh.requires_grad_(True), illu, refl, target=target.requires_grad_(True))


def test_train_step_lowers_the_reconstruction_term():
    from losses.loss import TotalLoss
    from models.model import MultiScaleUP_Retinex
    from trainers.train import make_optimizer, train_step
    torch.manual_seed(0)
    model = MultiScaleUP_Retinex(use_preact=False, use_aspp=False).to(DEV).train()
    crit = TotalLoss(weight_exp=0.0, weight_smooth=0.0, weight_col=0.0, weight_spa=0.0, weight_decouple=0.0,
                     weight_perceptual=0.0, weight_freq=0.0, use_freq_loss=False, use_dynamic_smooth_weight=False,
                     weight_rec=1.0, weight_ssim=1.0).to(DEV)
    opt = make_optimizer(model, lr=1e-3)
    low, _, _, _, target = _inputs(seed=3)
    rec = []
    for _ in range(10):
        loss, d = train_step(model, low, crit, opt, target=target)
        rec.append(d["reconstruction"])
        assert d["total"] == pytest.approx(d["reconstruction"] + d["ssim_loss"], rel=1e-6)
    print("reconstruction over 10 steps:", " ".join(f"{v:.5f}" for v in rec))
    assert all(math.isfinite(v) for v in rec) and rec[-1] < rec[0]


def test_paired_loader_gives_the_target_the_samples_geometry(tmp_path):
    """Identical files on both sides and no photometric stage: every (low, target) pair is equal bit for
    bit although the samples are flipped and rotated; with the photometric chain only the low side changes."""
    from datasets.dataset import get_train_dataloader
    low, gt = tmp_path / "low", tmp_path / "gt"
    low.mkdir()
    gt.mkdir()
    rng = np.random.default_rng(2)
    for i in range(6):
        img = Image.fromarray(rng.integers(0, 256, (48, 40, 3)).astype(np.uint8))
        img.save(low / f"p{i}.png")
        img.save(gt / f"p{i}.png")
    plain = get_train_dataloader(str(low), batch_size=3, image_size=64, num_workers=2, device=DEV, seed=4)
    paired = get_train_dataloader(str(low), batch_size=3, image_size=64, num_workers=2, device=DEV, seed=4,
                                  reference_dir=str(gt))
    adv = get_train_dataloader(str(low), batch_size=3, image_size=64, num_workers=0, device=DEV, seed=4,
                               reference_dir=str(gt), advanced_augment=True)
    batches = list(zip(plain, paired, adv))
    assert len(batches) == 2
    for x, (a, t), (a2, t2) in batches:
        assert a.shape == t.shape == (3, 3, 64, 64)
        assert torch.equal(a, x), "the low-light stream of a seeded run changed"
        assert torch.equal(t, a), "the target did not get the sample's flips and rot90"
        # the advanced loader draws other flips for the same images: its targets hold the same pixels, moved
        assert torch.equal(t2.flatten(1).sort(dim=1).values, t.flatten(1).sort(dim=1).values)
        assert not torch.equal(a2, t2), "only the low-light input is degraded further"


def test_main_train_with_a_reference_dir(tmp_path):
    import main as cli
    low, gt = tmp_path / "low", tmp_path / "gt"
    low.mkdir()
    gt.mkdir()
    rng = np.random.default_rng(5)
    for i in range(4):
        img = rng.integers(0, 256, (48, 40, 3))
        Image.fromarray(img.astype(np.uint8)).save(gt / f"im{i}.png")
        Image.fromarray((img * 0.3).astype(np.uint8)).save(low / f"im{i}.png")
    base = ["--mode", "train", "--train_dir", str(low), "--num_epochs", "1", "--batch_size", "2", "--image_size", "64",
            "--num_workers", "2", "--seed", "0", "--device", DEV]
    cli.main(base + ["--train_reference_dir", str(gt), "--save_dir", str(tmp_path / "paired")])
    rows = list(csv.DictReader(open(tmp_path / "paired" / "results.csv")))
    assert len(rows) == 1 and list(rows[0]) == ["epoch"] + KEYS + ["reconstruction", "ssim_loss"]
    assert all(math.isfinite(float(v)) for v in rows[0].values())
    assert float(rows[0]["reconstruction"]) > 0 and 0 < float(rows[0]["ssim_loss"]) < 1
    cli.main(base + ["--save_dir", str(tmp_path / "plain")])
    rows = list(csv.DictReader(open(tmp_path / "plain" / "results.csv")))
    assert len(rows) == 1 and list(rows[0]) == ["epoch"] + KEYS
