"""datasets/dataset.py without a device: draw_params consumes `random` in the
reference's order (pinned by the reference's own float64 outputs in
tests/golden/g9_augment*.npz), the record packing, and the restatements the GPU
tests compare against (aug_ref.py: the chain, the index map, Philox4x32-10)."""
import random

import numpy as np
import pytest
import torch

import aug_ref
from conftest import GOLDEN
from datasets import dataset as D
from upr import _lib as L
from upr import augment as uaug

CASES, REF_ERR = aug_ref.load_fixture(GOLDEN)


def test_fixture_holds_the_extreme_seeds():
    seeds = {c["seed"] for c in CASES if c["key"] == "a"}
    assert seeds == set(range(34))
    assert {4, 33} <= {c["seed"] for c in CASES if c["key"] == "b"}
    assert CASES[0]["x"].shape == (3, 40, 40) and CASES[-1]["x"].shape == (3, 33, 47)
    assert 0 < REF_ERR < 1e-6
    for c in CASES:
        assert np.abs(c["out32"].astype(np.float64) - c["out64"]).max() <= REF_ERR


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c['key']}{c['seed']}")
def test_draw_order_and_chain_match_reference(case):
    random.seed(case["seed"])
    p = D.draw_params(False, True)
    assert (p["hflip"], p["vflip"], p["k"]) == (False, False, 0)
    if case["seed"] == 33:
        assert aug_ref.stage_pattern(p) == (True,) * 6
    if case["seed"] == 4:
        assert aug_ref.stage_pattern(p) == (False,) * 6
    out = aug_ref.chain(case["x"], case["noise"], p)
    err = np.abs(out - case["out64"]).max()
    assert err <= 1e-12, err


class _Recorder:
    """A stand-in `random` that records the calls and answers from a script."""

    def __init__(self, answers):
        self.answers, self.calls = list(answers), []

    def random(self):
        self.calls.append("random")
        return self.answers.pop(0)

    def choice(self, seq):
        self.calls.append(("choice", tuple(seq)))
        return seq[1]

    def uniform(self, a, b):
        self.calls.append(("uniform", a, b))
        return (a + b) / 2


def test_geometric_draws_by_construction():
    r = _Recorder([0.6, 0.4, 0.7])
    p = D.draw_params(True, False, rng=r)
    assert r.calls == ["random", "random", "random", ("choice", (1, 2, 3))]
    assert (p["hflip"], p["vflip"], p["k"]) == (True, False, 2)
    r = _Recorder([0.5, 0.9, 0.5])  # > 0.5 is strict; no rotation -> no choice
    p = D.draw_params(True, False, rng=r)
    assert r.calls == ["random", "random", "random"]
    assert (p["hflip"], p["vflip"], p["k"]) == (False, True, 0)
    assert D.draw_params(False, False, rng=_Recorder([])) == {
        "hflip": False, "vflip": False, "k": 0, "gamma": None, "contrast": None, "brightness": None,
        "noise_level": None, "saturation": None, "shift": None}


def test_advanced_draws_by_construction():
    # geometry first (rotation fires), then each stage's decision, its uniform only when it fires
    r = _Recorder([0.1, 0.1, 0.9, 0.9, 0.1, 0.9, 0.31, 0.5, 0.51])
    p = D.draw_params(True, True, rng=r)
    assert r.calls == ["random", "random", "random", ("choice", (1, 2, 3)),
                       "random", ("uniform", 0.6, 1.8), "random", "random", ("uniform", -0.1, 0.1),
                       "random", ("uniform", 0.01, 0.03), "random", "random", ("uniform", -0.05, 0.05)]
    assert aug_ref.stage_pattern(p) == (True, False, True, True, False, True)
    r = _Recorder([0.9, 0.9, 0.9, 0.3, 0.9, 0.9])  # noise: > 0.3 is strict
    p = D.draw_params(False, True, rng=r)
    assert aug_ref.stage_pattern(p) == (True, True, True, False, True, True)
    assert r.calls[6] == "random" and len(r.calls) == 11


def test_global_random_is_the_default_source():
    random.seed(5)
    a = D.draw_params(True, True)
    b = D.draw_params(True, True, rng=random.Random(5))
    assert a == b


def test_pack_matches_c_record():
    p = {"hflip": True, "vflip": False, "k": 3, "gamma": 1.5, "contrast": None, "brightness": -0.05,
         "noise_level": 0.02, "saturation": None, "shift": 0.01}
    host = uaug.pack([D.draw_params(False, False), p], [7, 2 ** 40 + 3], pin=False)
    rec = (L.UprAugParams * 2).from_buffer_copy(host.numpy().tobytes())
    assert rec[0].flags == 0 and rec[0].sample_id == 7
    assert rec[1].flags == (L.UPR_AUG_HFLIP | 3 << L.UPR_AUG_ROT_SHIFT | L.UPR_AUG_GAMMA | L.UPR_AUG_BRIGHTNESS
                            | L.UPR_AUG_NOISE | L.UPR_AUG_SHIFT)
    assert rec[1].gamma == np.float32(1.5) and rec[1].brightness == np.float32(-0.05)
    assert rec[1].noise_level == np.float32(0.02) and rec[1].shift == np.float32(0.01)
    assert rec[1].contrast == 0 and rec[1].saturation == 0 and rec[1].sample_id == 2 ** 40 + 3
    assert uaug.out_shape(rec[1].flags, 48, 80) == (80, 48) and uaug.out_shape(rec[0].flags, 48, 80) == (48, 80)


def test_entries_validate_before_the_device():
    lib = L.lib()
    assert lib.upr_augment_workspace(8, 640, 640) >= 8 * 3 * 100 * 8
    assert lib.upr_augment_workspace(0, 64, 64) == 0
    assert lib.upr_augment(None, None, 1, 8, 8, None, None, 0, None, None, 0, None) == L.UPR_ERR_ARG
    assert lib.upr_augment_normals(None, 1, 8, 8, None, 0, None) == L.UPR_ERR_ARG


@pytest.mark.parametrize("shape", [(3, 5, 7), (3, 6, 6)])
def test_index_map_restatement_is_torch_flip_rot90(shape):
    x = torch.arange(int(np.prod(shape)), dtype=torch.float32).reshape(shape)
    for hf in (False, True):
        for vf in (False, True):
            for k in range(4):
                t = torch.flip(x, dims=[2]) if hf else x
                t = torch.flip(t, dims=[1]) if vf else t
                t = torch.rot90(t, k=k, dims=[1, 2]) if k else t
                np.testing.assert_array_equal(aug_ref.geometry(x.numpy(), hf, vf, k), t.numpy(), err_msg=(hf, vf, k))


def test_philox_known_answers():
    """Random123 philox4x32-10 known-answer vectors (counter, key -> output)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = tuple(int(v) for v in aug_ref.philox4x32_10(ctr, key))
        assert got == want, [hex(v) for v in got]


def test_normals_restatement_shape_and_moments():
    z = aug_ref.normals(3, 7, 33, 47)
    assert z.shape == (3, 33, 47) and np.isfinite(z).all() and np.abs(z).max() <= 6.8
    n = z.size
    assert abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1) <= 5 * np.sqrt(2 / n)


def test_loader_batching_without_decoding(tmp_path):
    from PIL import Image
    for i in range(7):
        Image.fromarray(np.full((8, 8, 3), i, np.uint8)).save(tmp_path / f"im{i}.png")
    (tmp_path / "notes.txt").write_text("x")
    ld = D.get_train_dataloader(str(tmp_path), batch_size=2, image_size=64, num_workers=2, seed=1)
    assert len(ld) == 4 and ld.batch_size == 2 and len(ld.dataset) == 7
    assert len(D.get_train_dataloader(str(tmp_path), batch_size=2, drop_last=True, seed=1)) == 3
    assert ld._order(0) == ld._order(0) and sorted(ld._order(0)) == list(range(7))
    assert ld._order(0) != ld._order(1)
    assert ld.dataset.image_files == sorted(ld.dataset.image_files)
    with pytest.raises(ValueError):
        D.LowLightDataset(str(tmp_path / "none"))
