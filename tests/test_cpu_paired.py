"""Paired training without a device: the float64 restatement of the two terms
and its closed-form gradient (tests/paired_ref.py) against torch autograd, its
SSIM against the metrics restatement, and the host side of the data path and
the CLI (stem matching, the pair checks, the target's augmentation records, the
parameter draws, the flag rules)."""
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

import metrics_ref
import paired_ref as R

AUTOGRAD_SHAPES = ((2, 7, 9), (1, 16, 16), (2, 37, 53))
# two float64 evaluations (shifted-slice sums here, avg_pool2d in torch) agree to 1e-12 relative.  On the
# near-constant pair the window (co)variances, ~1e-7, are differences of second moments of 0.25 and sit
# beside C2 = 9e-4 in the quotient: each evaluation carries 0.25 / C2 ~ 300 times the rounding of the
# other pairs, so that pair is held to 1e-10
AUTOGRAD_RTOL = {"noise": 1e-12, "smooth": 1e-12, "dark": 1e-12, "near_constant": 1e-10}


@pytest.mark.parametrize("shape", AUTOGRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", R.KINDS)
def test_closed_form_matches_float64_autograd(shape, kind):
    x, y = R.make_pair(kind, shape)
    eps = R.f32_eps()
    xt = torch.from_numpy(x).double().requires_grad_(True)
    yt = torch.from_numpy(y).double()
    rec, sl = R.torch_terms(xt, yt, eps)
    w_rec, w_ssim = 0.7, 1.3
    (w_rec * rec + w_ssim * sl).backward()
    r_rec, r_sl = R.terms(x, y, eps)
    rtol = AUTOGRAD_RTOL[kind]
    assert abs(r_rec - rec.item()) <= 1e-12 * abs(rec.item())
    # the term is formed as 1 - mean SSIM: two float64 evaluations of it differ by their error in
    # the mean SSIM (the window variances cancel), so the relative bound is on the larger of the two
    print(f"PAIRED cpu {kind} {shape}: ssim_loss {sl.item():.6e} |d| {abs(r_sl - sl.item()):.3e}")
    assert abs(r_sl - sl.item()) <= rtol * max(abs(sl.item()), abs(1.0 - sl.item()))
    g, ga = R.grad(x, y, w_rec, w_ssim, eps), xt.grad.numpy()
    print(f"PAIRED cpu {kind} {shape}: grad max|d| / max|g| {np.abs(g - ga).max() / np.abs(ga).max():.3e}")
    assert np.abs(g - ga).max() <= rtol * np.abs(ga).max()


@pytest.mark.parametrize("shape", ((1, 7, 9), (1, 37, 53)), ids=lambda s: "x".join(map(str, s)))
def test_ssim_is_the_metrics_ssim(shape):
    x, y = R.make_pair("smooth", shape)
    _, sl = R.terms(x, y)
    m = metrics_ref.metrics(x[0], y[0])[0][metrics_ref.NAMES.index("ssim")]
    assert metrics_ref.rel(1.0 - sl, m) <= metrics_ref.TOL_EXACT


def _png(path, h, w, seed):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)).save(path)


@pytest.fixture
def pair_dirs(tmp_path):
    low, gt = str(tmp_path / "low"), str(tmp_path / "gt")
    for i, stem in enumerate(("a", "b", "c")):
        _png(os.path.join(low, f"{stem}.png"), 20, 24, i)
        _png(os.path.join(gt, f"{stem}.png"), 20, 24, 10 + i)
    _png(os.path.join(gt, "unused.png"), 20, 24, 99)
    return low, gt


def test_stem_matching(pair_dirs, tmp_path):
    from datasets.dataset import PairedLowLightDataset, match_by_stem
    low, gt = pair_dirs
    os.remove(os.path.join(gt, "b.png"))
    _png(os.path.join(gt, "b.bmp"), 20, 24, 11)  # the stem decides, not the extension
    ds = PairedLowLightDataset(low, gt, image_size=32)
    assert [os.path.basename(f) for f in ds.image_files] == ["a.png", "b.png", "c.png"]
    assert [os.path.basename(f) for f in ds.reference_files] == ["a.png", "b.bmp", "c.png"]
    assert match_by_stem(["x/q.jpg"], ["y/q.png", "y/r.png"], "y") == ["y/q.png"]


def test_missing_ground_truth(pair_dirs):
    from datasets.dataset import PairedLowLightDataset
    from trainers.train import make_val_loaders
    low, gt = pair_dirs
    os.remove(os.path.join(gt, "c.png"))
    with pytest.raises(ValueError, match=r"no ground truth in .* for .*c\.png.* \(matched by file stem\)") as e1:
        PairedLowLightDataset(low, gt)
    with pytest.raises(ValueError) as e2:  # the validation loaders share the helper: the same error
        make_val_loaders(low, gt)
    assert str(e1.value) == str(e2.value)


def test_size_mismatch_names_both_files(pair_dirs):
    from datasets.dataset import DeviceLoader, PairedLowLightDataset, decode_pair, decode_u8
    low, gt = pair_dirs
    _png(os.path.join(gt, "b.png"), 20, 25, 5)
    ds = PairedLowLightDataset(low, gt, image_size=32)
    with pytest.raises(ValueError, match=r"low/b\.png.*gt/b\.png"):
        decode_pair(ds.image_files[1], ds.reference_files[1])
    decode_pair(ds.image_files[0], ds.reference_files[0])
    loader = DeviceLoader(ds, batch_size=3, shuffle=False, num_workers=0, seed=1)
    images = [decode_u8(f) for f in ds.image_files]
    targets = [decode_u8(f) for f in ds.reference_files]
    with pytest.raises(ValueError, match=r"low/b\.png.*gt/b\.png"):  # before anything touches a device
        loader._assemble([0, 1, 2], images, 0, random.Random(0), torch.device("cpu"), targets)


def test_target_records_carry_geometry_only():
    from datasets.dataset import draw_params
    from upr import _lib as L
    from upr import augment as uaug
    rng = random.Random(3)
    params = [draw_params(True, True, rng) for _ in range(64)]
    ids = list(range(100, 164))
    low = uaug.pack(params, ids, pin=False).numpy().view(uaug.RECORD)
    tgt = uaug.target_records(params, ids, pin=False).numpy().view(uaug.RECORD)
    geometry = L.UPR_AUG_HFLIP | L.UPR_AUG_VFLIP | (3 << L.UPR_AUG_ROT_SHIFT)
    photometric = 0
    for _, bit in uaug.STAGES:
        photometric |= bit
    assert (low["flags"] & photometric).any() and (low["flags"] & geometry).any()
    assert np.array_equal(tgt["flags"], low["flags"] & geometry)
    assert not (tgt["flags"] & photometric).any()
    assert np.array_equal(tgt["sample_id"], low["sample_id"])
    for name, _ in uaug.STAGES:
        assert not tgt[name].any()


def test_seeded_paired_loader_draws_the_unpaired_parameters(pair_dirs):
    from datasets.dataset import get_train_dataloader
    low, gt = pair_dirs
    a = get_train_dataloader(low, batch_size=2, image_size=32, advanced_augment=True, seed=11)
    b = get_train_dataloader(low, batch_size=2, image_size=32, advanced_augment=True, seed=11, reference_dir=gt)
    assert hasattr(b.dataset, "reference_files") and not hasattr(a.dataset, "reference_files")
    for epoch in (0, 3):
        (ba, ra), (bb, rb) = a._plan(epoch), b._plan(epoch)
        assert ba == bb
        for idxs in ba:
            assert a._draw(len(idxs), ra) == b._draw(len(idxs), rb)


def test_cli_rules(capsys):
    import main
    base = ["--mode", "train", "--train_dir", "D"]
    a = main.parse_args(base)
    assert a.train_reference_dir is None and a.weight_rec is None and a.weight_ssim is None and a.rec_eps == 1e-3
    a = main.parse_args(base + ["--train_reference_dir", "G"])
    assert (a.weight_rec, a.weight_ssim, a.rec_eps) == (1.0, 1.0, 1e-3)
    a = main.parse_args(base + ["--train_reference_dir", "G", "--weight_rec", "0.25", "--rec_eps", "1e-2"])
    assert (a.weight_rec, a.weight_ssim, a.rec_eps) == (0.25, 1.0, 1e-2)
    for flag in ("--weight_rec", "--weight_ssim"):
        with pytest.raises(SystemExit):
            main.parse_args(base + [flag, "1.0"])
        assert f"{flag} needs --train_reference_dir" in capsys.readouterr().err


def test_driver_rules():
    from trainers import train as T
    assert T.paired_weights(None) == (0.0, 0.0)
    assert T.paired_weights("G") == (1.0, 1.0)
    assert T.paired_weights("G", 0.5, None) == (0.5, 1.0)
    with pytest.raises(ValueError, match="--weight_ssim needs --train_reference_dir"):
        T.paired_weights(None, None, 2.0)
    T.check_best_by("val_ssim", True, True)
    with pytest.raises(ValueError, match="--best_by val_ssim needs --val_reference_dir"):
        T.check_best_by("val_ssim", True, False)
    with pytest.raises(ValueError, match="--best_by val_ssim needs --val_dir"):
        T.check_best_by("val_ssim", False, False)
    t = T.BestTracker("val_ssim")
    assert t.update(1.0, {"val_ssim": 0.5}) is True
    assert t.update(1.0, {"val_ssim": 0.4}) is False and t.counter == 1
    assert t.update(1.0, {"val_ssim": 0.6}) is True and t.best == 0.6
    assert T.PAIRED_KEYS == ("reconstruction", "ssim_loss")


def test_loss_surface():
    import inspect

    from losses import loss as LS
    from upr import loss_engine as E
    sig = inspect.signature(LS.TotalLoss.__init__).parameters
    assert (sig["weight_rec"].default, sig["weight_ssim"].default, sig["rec_eps"].default) == (0.0, 0.0, 1e-3)
    # forward keeps the reference's five parameters (test_cpu_train_surface.py); the target is a keyword of the call
    assert inspect.signature(LS.TotalLoss.__call__).parameters["target"].default is None
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="ROCm devices only"):  # the paired path refuses CPU tensors as well
        LS.TotalLoss()(x, x, x[:, :1], x, target=x)
    assert inspect.signature(E.TotalLossEngine.__call__).parameters["target"].default is None
    assert inspect.signature(LS.ReconstructionLoss.__init__).parameters["eps"].default == 1e-3
    assert list(inspect.signature(LS.SSIMLoss.forward).parameters) == ["self", "img_enhanced", "target"]
    from trainers.train import train_step
    assert inspect.signature(train_step).parameters["target"].default is None
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        LS.SSIMLoss()(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))
