"""The device-free pieces of validation in --mode train: the new flags and the
--best_by argument errors, the best / patience rule, and results.csv with and
without val_* columns."""
import csv

import pytest

from trainers import train as T

KEYS = ["total", "exposure", "smoothness", "color", "spatial", "decouple", "perceptual"]


def test_parser_defaults_are_inert():
    import main as cli
    a = cli.parse_args(["--mode", "train"])
    assert a.val_dir is None and a.val_reference_dir is None and a.val_freq == 1 and a.val_batch_size is None
    assert a.best_by == "train_total" and a.val_samples == 4 and a.lowlight_dir is None and a.loe_size == 50


def test_parser_accepts_the_validation_flags():
    import main as cli
    a = cli.parse_args(["--mode", "train", "--val_dir", "v", "--val_reference_dir", "g", "--val_freq", "3",
                        "--val_batch_size", "5", "--best_by", "val_psnr", "--val_samples", "0", "--loe_size", "0"])
    assert (a.val_dir, a.val_reference_dir, a.val_freq, a.val_batch_size) == ("v", "g", 3, 5)
    assert (a.best_by, a.val_samples, a.loe_size) == ("val_psnr", 0, 0)
    for by in ("val_total", "val_loe", "train_total"):
        assert cli.parse_args(["--mode", "train", "--val_dir", "v", "--best_by", by]).best_by == by
    a = cli.parse_args(["--mode", "evaluate", "--lowlight_dir", "low", "--loe_size", "16"])
    assert a.lowlight_dir == "low" and a.loe_size == 16


@pytest.mark.parametrize("argv,needs", [
    (["--best_by", "val_total"], "--val_dir"),
    (["--best_by", "val_loe"], "--val_dir"),
    (["--best_by", "val_psnr"], "--val_dir"),
    (["--best_by", "val_psnr", "--val_dir", "v"], "--val_reference_dir"),
    (["--val_reference_dir", "g"], "--val_dir"),
    (["--best_by", "val_ssim", "--val_dir", "v"], "invalid choice"),
    (["--val_freq", "0", "--val_dir", "v"], "--val_freq"),
    (["--val_samples", "-1"], "--val_samples"),
    (["--loe_size", "-2"], "--loe_size"),
])
def test_parser_rejects_invalid_combinations(argv, needs, capsys):
    import main as cli
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--mode", "train"] + argv)
    assert e.value.code == 2 and needs in capsys.readouterr().err


def test_train_rejects_best_by_without_validation_before_the_device(monkeypatch):
    import argparse
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("device touched")))
    with pytest.raises(ValueError, match="--val_dir"):
        T.train(argparse.Namespace(best_by="val_loe", val_dir=None))
    with pytest.raises(ValueError, match="--val_reference_dir"):
        T.train(argparse.Namespace(best_by="val_psnr", val_dir="v", val_reference_dir=None))
    T.check_best_by("val_psnr", True, True)
    T.check_best_by("train_total", False, False)


def test_val_columns_order():
    cols = T.val_columns(False)
    assert cols == ["val_" + k for k in KEYS] + ["val_mean_brightness", "val_contrast", "val_entropy", "val_niqe",
                                                 "val_saturation", "val_naturalness", "val_loe"]
    assert T.val_columns(True) == ["val_" + k for k in KEYS] + [
        "val_mean_brightness", "val_contrast", "val_entropy", "val_niqe", "val_psnr", "val_ssim", "val_mse",
        "val_saturation", "val_naturalness", "val_loe"]


def test_best_tracker_train_total_is_todays_rule():
    t = T.BestTracker()
    got = [t.update(v, None) for v in (3.0, 2.0, 2.0, 2.5, 1.0)]
    assert got == [True, True, False, False, True] and t.best == 1.0 and t.counter == 0
    # validation numbers do not matter to train_total
    t = T.BestTracker("train_total")
    assert [t.update(v, {"val_loe": 9.0 - v}) for v in (3.0, 2.0, 2.5)] == [True, True, False] and t.counter == 1


def test_best_tracker_val_choice_skips_epochs_not_validated():
    t = T.BestTracker("val_loe")
    seq = [(5.0, {"val_loe": 10.0}), (4.0, None), (3.0, {"val_loe": 12.0}), (2.0, None), (1.0, {"val_loe": 9.0}),
           (0.5, {"val_loe": 9.0})]
    got = [t.update(tr, v) for tr, v in seq]
    assert got == [True, None, False, None, True, False]
    assert t.best == 9.0 and t.counter == 1
    # the counter neither advanced nor was reset on the epochs that were not validated
    t = T.BestTracker("val_total")
    assert t.update(1.0, {"val_total": 1.0}) is True and t.update(1.0, {"val_total": 2.0}) is False
    assert t.update(0.1, None) is None and t.counter == 1 and t.best == 1.0


def test_best_tracker_psnr_is_better_when_higher():
    t = T.BestTracker("val_psnr")
    got = [t.update(1.0, {"val_psnr": p}) for p in (20.0, 19.0, 21.0, 21.0)]
    assert got == [True, False, True, False] and t.best == 21.0 and t.counter == 1


def test_results_csv_without_val_columns_is_unchanged(tmp_path):
    hist = {k: [0.5 + i, 0.25 + i] for i, k in enumerate(KEYS)}
    a = T.save_results_to_csv(hist, str(tmp_path / "a"))
    b = T.save_results_to_csv(hist, str(tmp_path / "b"), None)
    text = open(a).read()
    assert text == open(b).read()
    assert text.splitlines()[0] == ",".join(["epoch"] + KEYS)
    assert text.splitlines()[1] == "0," + ",".join(str(0.5 + i) for i in range(len(KEYS)))


def test_results_csv_with_val_columns(tmp_path):
    hist = {k: [0.5, 0.25, 0.125] for k in KEYS}
    cols = T.val_columns(False)
    val = {c: [None, 1.0 / 3 + i, None] for i, c in enumerate(cols)}
    rows = list(csv.reader(open(T.save_results_to_csv(hist, str(tmp_path), val))))
    assert rows[0] == ["epoch"] + KEYS + cols
    assert rows[1][len(KEYS) + 1:] == [""] * len(cols) and rows[3][len(KEYS) + 1:] == [""] * len(cols)
    assert [float(v) for v in rows[2][len(KEYS) + 1:]] == [1.0 / 3 + i for i in range(len(cols))]
    assert [r[:len(KEYS) + 1] for r in rows[1:]] == [[str(e)] + [str(hist[k][e]) for k in KEYS] for e in range(3)]
