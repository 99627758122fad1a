"""The host side of the epoch driver (trainers/train.py) without a device: the
two schedulers against torch's, the checkpoint file format, results.csv and the
CLI's training flags."""
import csv

import pytest
import torch

from trainers import train as T


class _Opt:
    """What a scheduler needs of upr.optim.Adam: param_groups[0]['lr']."""

    def __init__(self, lr):
        self.param_groups = [{"lr": lr}]


def _torch_lrs(make, lr, epochs):
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    sched = make(opt)
    out = [opt.param_groups[0]["lr"]]
    for _ in range(epochs):
        opt.step()
        sched.step()
        out.append(opt.param_groups[0]["lr"])
    return out


def _our_lrs(make, lr, epochs):
    opt = _Opt(lr)
    sched = make(opt)
    out = [opt.param_groups[0]["lr"]]
    for _ in range(epochs):
        sched.step()
        out.append(opt.param_groups[0]["lr"])
    return out


def test_step_lr_matches_torch():
    want = _torch_lrs(lambda o: torch.optim.lr_scheduler.StepLR(o, step_size=30, gamma=0.5), 1e-4, 75)
    got = _our_lrs(lambda o: T.StepLR(o, step_size=30, gamma=0.5), 1e-4, 75)
    assert len(got) == 76 and got[30] == pytest.approx(5e-5, rel=1e-12) and got[29] == pytest.approx(1e-4, rel=1e-12)
    for e, (a, b) in enumerate(zip(got, want)):
        assert a == pytest.approx(b, rel=1e-12, abs=0), e


def test_cosine_warm_restarts_matches_torch():
    want = _torch_lrs(lambda o: torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(o, T_0=10, T_mult=2,
                                                                                      eta_min=1e-6), 1e-4, 75)
    got = _our_lrs(lambda o: T.CosineAnnealingWarmRestarts(o, T_0=10, T_mult=2, eta_min=1e-6), 1e-4, 75)
    assert got[10] == pytest.approx(1e-4, rel=1e-12) and got[30] == pytest.approx(1e-4, rel=1e-12)  # restarts
    assert got[70] == pytest.approx(1e-4, rel=1e-12) and min(got) > 1e-6
    for e, (a, b) in enumerate(zip(got, want)):
        assert a == pytest.approx(b, rel=1e-12, abs=0), e


def test_schedulers_resume_in_phase():
    full = _our_lrs(lambda o: T.StepLR(o, step_size=3, gamma=0.5), 1e-3, 10)
    opt = _Opt(123.0)  # a resumed optimizer's lr is whatever the checkpoint held
    s = T.StepLR(opt, step_size=3, gamma=0.5, last_epoch=4, base_lr=1e-3)
    assert opt.param_groups[0]["lr"] == full[4]
    s.step()
    s.step()
    assert opt.param_groups[0]["lr"] == full[6]


class _Adamish:
    def __init__(self):
        self.step_count, self.m, self.v = 0, torch.zeros(5), torch.zeros(5)
        self.param_groups = [{"lr": 1e-4, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 1e-5}]

    def state_dict(self):
        return {"step": self.step_count, "m": self.m, "v": self.v, "param_groups": [dict(self.param_groups[0])]}

    def load_state_dict(self, sd):
        self.step_count = int(sd["step"])
        self.m.copy_(sd["m"])
        self.v.copy_(sd["v"])
        self.param_groups[0].update(sd["param_groups"][0])


def test_checkpoint_round_trip(tmp_path):
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4))
    opt = _Adamish()
    opt.step_count, opt.param_groups[0]["lr"] = 17, 2.5e-5
    opt.m.normal_()
    opt.v.uniform_()
    T.save_checkpoint(model, opt, 6, str(tmp_path), is_best=False)
    assert (tmp_path / "latest_model.pth").exists() and not (tmp_path / "best_model.pth").exists()
    T.save_checkpoint(model, opt, 6, str(tmp_path), is_best=True)
    for name in ("latest_model.pth", "best_model.pth"):
        ck = torch.load(tmp_path / name, map_location="cpu", weights_only=True)
        assert sorted(ck) == ["epoch", "model_state_dict", "optimizer_state_dict"] and ck["epoch"] == 6
        assert list(ck["model_state_dict"]) == list(model.state_dict())
    model2 = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4))
    opt2 = _Adamish()
    assert T.load_checkpoint(model2, opt2, str(tmp_path / "latest_model.pth"), map_location="cpu") == 7
    for (k, a), b in zip(model.state_dict().items(), model2.state_dict().values()):
        assert torch.equal(a, b), k
    assert opt2.step_count == 17 and opt2.param_groups[0]["lr"] == 2.5e-5
    assert opt2.param_groups[0]["betas"] == (0.9, 0.999)
    assert torch.equal(opt2.m, opt.m) and torch.equal(opt2.v, opt.v)
    with pytest.raises(FileNotFoundError):
        T.load_checkpoint(model2, opt2, str(tmp_path / "missing.pth"))


def test_results_csv(tmp_path):
    hist = {k: [1.0 + i, 0.5 + i] for i, k in enumerate(T.LOSS_KEYS)}
    path = T.save_results_to_csv(hist, str(tmp_path))
    rows = list(csv.DictReader(open(path)))
    assert len(rows) == 2 and list(rows[0]) == ["epoch"] + list(T.LOSS_KEYS)
    assert rows[1]["epoch"] == "1" and float(rows[1]["perceptual"]) == 6.5
    assert T.LOSS_KEYS == ('total', 'exposure', 'smoothness', 'color', 'spatial', 'decouple', 'perceptual')


def test_cli_accepts_the_training_flags():
    import main as cli
    argv = ["--mode", "train", "--train_dir", "d", "--save_dir", "s", "--num_epochs", "2", "--batch_size", "2",
            "--image_size", "64", "--num_workers", "3", "--lr", "2e-4", "--weight_decay", "1e-6",
            "--lr_decay_step", "1", "--lr_decay_gamma", "0.25", "--weight_exp", "9", "--weight_smooth", "2",
            "--weight_col", "0.4", "--weight_spa", "1.5", "--weight_decouple", "0.2", "--weight_perceptual", "0.9",
            "--weight_freq", "0.3", "--resume", "r.pth", "--use_amp", "--patience", "5", "--use_cosine_scheduler",
            "--advanced_augment", "--use_freq_loss", "--adaptive_weights"]
    a = cli.build_parser().parse_args(argv)
    assert a.mode == "train" and a.image_size == 64 and a.num_workers == 3 and a.lr == 2e-4
    assert a.weight_decay == 1e-6 and a.lr_decay_step == 1 and a.lr_decay_gamma == 0.25
    assert (a.weight_exp, a.weight_smooth, a.weight_col, a.weight_spa) == (9, 2, 0.4, 1.5)
    assert (a.weight_decouple, a.weight_perceptual, a.weight_freq) == (0.2, 0.9, 0.3)
    assert a.resume == "r.pth" and a.patience == 5
    assert a.use_amp and a.use_cosine_scheduler and a.advanced_augment and a.use_freq_loss and a.adaptive_weights
    d = cli.build_parser().parse_args(["--mode", "train"])
    assert (d.image_size, d.num_workers, d.lr, d.weight_decay, d.lr_decay_step, d.lr_decay_gamma, d.patience) == \
        (640, 4, 1e-4, 1e-5, 30, 0.5, 20)
    assert callable(__import__("trainers.train", fromlist=["train"]).train)
