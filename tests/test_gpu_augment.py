"""The device augmentation (csrc/augment.hip via upr.augment / datasets.dataset):
the photometric chain against the reference's own outputs, the flip / rot90
index map against torch, the Philox noise generator against its float64
restatement, the statistics pass, and the loader end to end."""
import random

import numpy as np
import pytest
import torch
from PIL import Image

import aug_ref
from conftest import GOLDEN, has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]
DEV = "cuda:0"
CASES, REF_ERR = aug_ref.load_fixture(GOLDEN)
OFF = {"hflip": False, "vflip": False, "k": 0, "gamma": None, "contrast": None, "brightness": None,
       "noise_level": None, "saturation": None, "shift": None}


def _aug(x, params, ids=None, seed=0, noise=None, out=None):
    from upr import augment as A
    ids = list(range(len(params))) if ids is None else ids
    return A.augment(x, A.pack(params, ids), seed=seed, noise=noise, out=out)


def _geo(hf, vf, k):
    return dict(OFF, hflip=hf, vflip=vf, k=k)


def _torch_geo(x, p):
    t = torch.flip(x, dims=[2]) if p["hflip"] else x
    t = torch.flip(t, dims=[1]) if p["vflip"] else t
    return torch.rot90(t, k=p["k"], dims=[1, 2]) if p["k"] else t


# ---- the chain against the reference ---------------------------------------------------------

def test_chain_matches_reference_fixture():
    """Every fixture seed: the device output with the reference's own noise draw and
    draw_params' record is within 4 x ref_err (absolute, values in [0, 1]) of the
    reference's float64 output.  The margin covers the device powf and the
    fp64-ordered mean against torch's fp32 ones; every later stage has gain <= 1.2."""
    from datasets.dataset import draw_params
    worst = 0.0
    for c in CASES:
        random.seed(c["seed"])
        p = draw_params(False, True)
        x = torch.from_numpy(c["x"]).to(DEV)[None]
        y = _aug(x, [p], noise=torch.from_numpy(c["noise"]).to(DEV)[None])
        err = float(np.abs(y[0].cpu().numpy().astype(np.float64) - c["out64"]).max())
        worst = max(worst, err)
        assert err <= 4 * REF_ERR, (c["key"], c["seed"], err, REF_ERR)
    print(f"device chain: max |d| vs the reference's float64 output {worst:.3e} (ref_err {REF_ERR:.3e}, "
          f"bound {4 * REF_ERR:.3e}) over {len(CASES)} cases")


# ---- geometry -------------------------------------------------------------------------------

ALL16 = [(hf, vf, k) for hf in (False, True) for vf in (False, True) for k in range(4)]


@pytest.mark.parametrize("shape,combos", [((3, 40, 40), ALL16),
                                          ((3, 33, 47), [c for c in ALL16 if c[2] % 2 == 0]),
                                          ((3, 64, 128), [c for c in ALL16 if c[2] % 2 == 0]),
                                          ((3, 33, 47), [c for c in ALL16 if c[2] % 2 == 1]),
                                          ((3, 64, 128), [c for c in ALL16 if c[2] % 2 == 1])],
                         ids=["40x40", "33x47-even", "64x128-even", "33x47-odd", "64x128-odd"])
def test_geometry_bit_exact(shape, combos):
    x = torch.rand(shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    for hf, vf, k in combos:
        p = _geo(hf, vf, k)
        y = _aug(x[None], [p])[0]
        want = _torch_geo(x, p)
        assert y.shape == want.shape and torch.equal(y, want), (shape, hf, vf, k)


@pytest.mark.parametrize("ks", [(0, 2, 0, 2, 2), (1, 3, 3, 1, 1)], ids=["even", "odd"])
def test_geometry_batch_of_five_records(ks):
    x = torch.rand((5, 3, 33, 48), generator=torch.Generator().manual_seed(4)).to(DEV)
    ps = [_geo(bool(i & 1), bool(i & 2), k) for i, k in enumerate(ks)]
    y = _aug(x, ps)
    for i, p in enumerate(ps):
        assert torch.equal(y[i], _torch_geo(x[i], p)), i


def test_square_batch_may_mix_odd_and_even():
    x = torch.rand((4, 3, 40, 40), generator=torch.Generator().manual_seed(5)).to(DEV)
    ps = [_geo(True, False, 1), _geo(False, True, 0), _geo(False, False, 3), _geo(True, True, 2)]
    y = _aug(x, ps)
    for i, p in enumerate(ps):
        assert torch.equal(y[i], _torch_geo(x[i], p)), i


def test_mixed_shapes_refused_before_launch():
    from upr import _lib as L
    from upr import augment as A
    x = torch.rand((2, 3, 48, 80), generator=torch.Generator().manual_seed(6)).to(DEV)
    out = torch.full((2, 3, 48, 80), -7.0, device=DEV)
    rec = A.pack([_geo(False, False, 0), _geo(False, False, 1)], [0, 1])
    with pytest.raises(RuntimeError, match="shape"):
        A.augment(x, rec, out=out)
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    lib = L.lib()
    ws = torch.empty(lib.upr_augment_workspace(2, 48, 80), dtype=torch.uint8, device=DEV)
    rd = rec.to(DEV)
    rc = lib.upr_augment(x.data_ptr(), out.data_ptr(), 2, 48, 80, rd.data_ptr(), rec.data_ptr(), 0, None,
                         ws.data_ptr(), ws.numel(), None)
    assert rc == L.UPR_ERR_SHAPE
    rc = lib.upr_augment(x.data_ptr(), out.data_ptr(), 2, 48, 80, rd.data_ptr(), rec.data_ptr(), 0, None,
                         ws.data_ptr(), 8, None)
    assert rc == L.UPR_ERR_SHAPE  # the shape check comes first
    torch.cuda.synchronize()
    assert (out == -7.0).all()


@pytest.mark.parametrize("p", [_geo(True, False, 0), _geo(False, True, 2), _geo(True, True, 1),
                               dict(OFF, hflip=True, gamma=1.3, contrast=1.2, brightness=0.05, noise_level=0.02,
                                    saturation=1.1, shift=-0.02)], ids=["hflip", "k2", "k1", "chain"])
def test_misaligned_input_same_bytes(p):
    g = torch.Generator().manual_seed(7)
    x = torch.rand((2, 3, 40, 64), generator=g).to(DEV)
    flat = torch.empty(x.numel() + 1, device=DEV)
    flat[1:] = x.reshape(-1)
    xm = flat[1:].view(x.shape)
    assert xm.data_ptr() % 16 == 4 and xm.is_contiguous()
    a = _aug(x, [p, p], ids=[3, 9], seed=11)
    b = _aug(xm, [p, p], ids=[3, 9], seed=11)
    assert torch.equal(a, b)


# ---- the noise generator (debug entry) --------------------------------------------------------

def test_normals_match_restatement():
    from upr import augment as A
    seed, sid = 0x1234567890ABCDEF, 2 ** 33 + 5
    z = A.normals([sid], 40, 40, seed, DEV)[0].cpu().numpy().astype(np.float64)
    want = aug_ref.normals(seed, sid, 40, 40)
    err = np.abs(z - want).max()
    print(f"normals vs float64 Philox + Box-Muller: max |d| {err:.3e}")
    assert err <= 1e-5
    z2 = A.normals([1], 33, 47, 5, DEV)[0].cpu().numpy().astype(np.float64)  # 3*33*47 % 4 != 0: a partial group
    assert np.abs(z2 - aug_ref.normals(5, 1, 33, 47)).max() <= 1e-5


def test_normals_depend_on_seed_and_sample_only():
    from upr import augment as A
    alone = A.normals([7], 40, 40, 99, DEV)
    assert torch.equal(alone, A.normals([7], 40, 40, 99, DEV))
    five = A.normals([0, 1, 2, 7, 4], 40, 40, 99, DEV)
    two = A.normals([7, 8], 40, 40, 99, DEV)
    assert torch.equal(five[3], alone[0]) and torch.equal(two[0], alone[0])
    assert not torch.equal(five[0], alone[0])
    assert not torch.equal(A.normals([7], 40, 40, 100, DEV), alone)


def test_normals_moments():
    from upr import augment as A
    z = A.normals(list(range(8)), 128, 128, 2024, DEV).double()
    n = z.numel()
    assert n == 393216
    mean, var = z.mean().item(), z.var(unbiased=False).item()
    zc = z - mean
    lag1 = ((zc[..., :-1] * zc[..., 1:]).mean() / var).item()
    print(f"normals: mean {mean:.3e}, var-1 {var - 1:.3e}, lag-1 {lag1:.3e} (5/sqrt(N) = {5 / n ** 0.5:.3e})")
    assert abs(mean) <= 5 / n ** 0.5
    assert abs(var - 1) <= 5 * (2 / n) ** 0.5
    assert abs(lag1) <= 5 / n ** 0.5


# ---- the whole chain with generated noise -----------------------------------------------------

@pytest.mark.parametrize("shape,k", [((3, 40, 40), 0), ((3, 40, 40), 1), ((3, 33, 47), 2), ((3, 33, 47), 3)],
                         ids=["vec", "transpose", "scalar", "transpose-ragged"])
def test_generated_noise_is_the_debug_entrys(shape, k):
    from upr import augment as A
    x = (torch.rand((2,) + shape, generator=torch.Generator().manual_seed(8)) * 0.5).to(DEV)
    p = dict(OFF, hflip=True, k=k, gamma=0.8, contrast=1.1, brightness=0.03, noise_level=0.03, saturation=0.9,
             shift=0.02)
    ids, seed = [12, 2 ** 40 + 1], 77
    a = _aug(x, [p, p], ids=ids, seed=seed)
    assert torch.equal(a, _aug(x, [p, p], ids=ids, seed=seed))
    Ho, Wo = a.shape[2:]
    z = A.normals(ids, Ho, Wo, seed, DEV)
    assert torch.equal(a, _aug(x, [p, p], ids=ids, seed=seed, noise=z))
    assert not torch.equal(a, _aug(x, [p, p], ids=ids, seed=seed + 1))
    assert a.min() >= 0 and a.max() <= 1


# ---- the statistics pass ------------------------------------------------------------------------

def _checkerboard(B, H, W):
    """Constant planes + a +-delta checkerboard: each channel's mean is its constant exactly."""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    sign = np.where((yy + xx) % 2 == 0, 1.0, -1.0).astype(np.float32)
    base = np.asarray([[0.25, 0.5, 0.75], [0.125, 0.375, 0.625], [0.5, 0.25, 0.0625]], np.float32)[:B]
    return base[:, :, None, None] + np.float32(0.0625) * sign[None, None]


@pytest.mark.parametrize("shape", [(64, 128), (33, 47)], ids=["64x128", "33x47"])
def test_contrast_alone(shape):
    H, W = shape
    x = _checkerboard(3, H, W)
    p = dict(OFF, contrast=1.2)
    xd = torch.from_numpy(x).to(DEV)
    runs = [_aug(xd, [p] * 3) for _ in range(3)]
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    got = runs[0].cpu().numpy().astype(np.float64)
    for b in range(3):
        want = aug_ref.chain(x[b], None, p)
        assert np.abs(got[b] - want).max() <= 1e-6, b
    if H * W % 2 == 0:  # the means are the constants: (v - m) * 1.2 + m in fp32, exactly
        m = x.mean(axis=(2, 3), keepdims=True, dtype=np.float64).astype(np.float32)
        assert np.array_equal(runs[0].cpu().numpy(), np.clip((x - m) * np.float32(1.2) + m, 0, 1))


def test_contrast_only_where_its_bit_is_set():
    x = torch.from_numpy(_checkerboard(3, 64, 128)).to(DEV)
    y = _aug(x, [dict(OFF, contrast=1.2), OFF, dict(OFF, gamma=1.5, contrast=0.8)])
    assert torch.equal(y[1], x[1])
    want = aug_ref.chain(x[2].cpu().numpy(), None, dict(OFF, gamma=1.5, contrast=0.8))
    assert np.abs(y[2].cpu().numpy() - want).max() <= 1e-6


def test_getitem_is_a_batch_of_one(tmp_path):
    from datasets.dataset import LowLightDataset, draw_params
    from utils.letterbox import letterbox_u8_image
    img = np.random.default_rng(2).integers(0, 120, (64, 64, 3), dtype=np.uint8)
    Image.fromarray(img).save(tmp_path / "a.png")
    ds = LowLightDataset(str(tmp_path), image_size=64)
    ds.seed = 5
    random.seed(21)
    got = ds[0]
    random.seed(21)
    p = draw_params(True, True)
    base = letterbox_u8_image(img, 64, auto=True, scaleup=True, device=torch.device(DEV))[0]
    assert got.device.type == "cuda" and got.dtype == torch.float32
    assert torch.equal(got, _aug(base[None], [p], ids=[0], seed=5)[0])


# ---- the loader -------------------------------------------------------------------------------

def _write_pngs(folder, n, size=(64, 64), start=0):
    rng = np.random.default_rng(17)
    for i in range(start, start + n):
        Image.fromarray(rng.integers(0, 140, size + (3,), dtype=np.uint8)).save(folder / f"im{i:02d}.png")


def _collect(loader, epoch=0):
    loader.set_epoch(epoch)
    return [b for b in loader]


def test_loader_batches(tmp_path):
    from datasets.dataset import get_train_dataloader
    _write_pngs(tmp_path, 7)
    for adv, drop, want in ((False, False, [2, 2, 2, 1]), (True, False, [2, 2, 2, 1]), (True, True, [2, 2, 2])):
        ld = get_train_dataloader(str(tmp_path), batch_size=2, image_size=64, num_workers=2, seed=1,
                                  advanced_augment=adv, drop_last=drop)
        a = _collect(ld)
        assert [b.shape[0] for b in a] == want and len(ld) == len(want)
        for b in a:
            assert b.shape[1:] == (3, 64, 64) and b.dtype == torch.float32 and b.device.type == "cuda"
            assert b.min() >= 0 and b.max() <= 1
        again = _collect(ld)
        assert all(torch.equal(p, q) for p, q in zip(a, again))
        other = _collect(ld, epoch=1)
        assert not all(torch.equal(p, q) for p, q in zip(a, other))


def test_loader_noise_does_not_depend_on_batch_size(tmp_path):
    """No geometric or photometric draw but the noise: a sample's pixels are fixed by (seed, epoch, index)."""
    from datasets.dataset import DeviceLoader, LowLightDataset
    _write_pngs(tmp_path, 5)
    import datasets.dataset as D
    keep = D.draw_params
    D.draw_params = lambda a, b, rng=None: dict(OFF, noise_level=0.03)
    try:
        outs = []
        for bs in (1, 2, 5):
            ld = DeviceLoader(LowLightDataset(str(tmp_path), image_size=64), batch_size=bs, shuffle=False, num_workers=0,
                              device=DEV, seed=3)
            ld.set_epoch(2)
            outs.append(torch.cat([b for b in ld]))
    finally:
        D.draw_params = keep
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert not torch.equal(outs[0][0], outs[0][1])


def test_loader_without_augmentation_is_the_letterbox(tmp_path):
    from datasets.dataset import DeviceLoader, LowLightDataset
    from utils.letterbox import letterbox_u8_image
    _write_pngs(tmp_path, 3, size=(48, 60))
    ds = LowLightDataset(str(tmp_path), image_size=64, augment=False, advanced_augment=False)
    ld = DeviceLoader(ds, batch_size=2, shuffle=False, num_workers=2, device=DEV, seed=0)
    got = torch.cat(_collect(ld))
    assert got.shape[0] == 3
    for i, f in enumerate(ds.image_files):
        img = np.asarray(Image.open(f).convert("RGB"))
        want = letterbox_u8_image(img, 64, auto=True, scaleup=True, device=torch.device(DEV))[0]
        assert torch.equal(got[i], want), f


def test_loader_names_files_of_a_ragged_batch(tmp_path):
    """A 64 x 96 image among 64 x 64 ones does NOT make a ragged batch: the
    reference's letterbox (auto=True: padding modulo 32) scales it to 43 x 64
    and pads 21 rows, 64 x 64 like the others, and its collate accepts it too.
    An image the letterbox does leave in another shape (64 x 128 -> 32 x 64:
    the 32 rows of padding vanish modulo 32) raises, naming the files."""
    from datasets.dataset import get_train_dataloader
    from utils.letterbox import letterbox_shape
    _write_pngs(tmp_path, 3)
    _write_pngs(tmp_path, 1, size=(64, 96), start=3)
    assert letterbox_shape((64, 96), 64) == (64, 64) and letterbox_shape((96, 64), 64) == (64, 64)
    ld = get_train_dataloader(str(tmp_path), batch_size=4, image_size=64, num_workers=2, seed=1, shuffle=False)
    assert [tuple(b.shape) for b in _collect(ld)] == [(4, 3, 64, 64)]
    _write_pngs(tmp_path, 1, size=(64, 128), start=4)
    assert letterbox_shape((64, 128), 64) == (32, 64)
    ld = get_train_dataloader(str(tmp_path), batch_size=5, image_size=64, num_workers=2, seed=1, shuffle=False)
    with pytest.raises(RuntimeError, match=r"im04\.png"):
        _collect(ld)
    # rot90 on a non-square batch: an odd and an even k cannot share a batch either
    import datasets.dataset as D
    for f in tmp_path.glob("im0[0-3].png"):
        f.unlink()
    _write_pngs(tmp_path, 1, size=(64, 128), start=5)
    draws = iter([dict(OFF, k=1), dict(OFF, k=2)])
    keep = D.draw_params
    D.draw_params = lambda a, b, rng=None: next(draws)
    try:
        ld = get_train_dataloader(str(tmp_path), batch_size=2, image_size=64, num_workers=0, seed=1, shuffle=False)
        with pytest.raises(RuntimeError, match=r"im04\.png k=1.*im05\.png k=2"):
            _collect(ld)
    finally:
        D.draw_params = keep


def test_test_dataset_and_loader(tmp_path):
    from datasets.dataset import LowLightTestDataset, get_test_dataloader
    from utils.letterbox import letterbox_u8_image
    _write_pngs(tmp_path, 3, size=(48, 60))
    ds = LowLightTestDataset(str(tmp_path))
    x, name = ds[1]
    img = np.asarray(Image.open(tmp_path / "im01.png").convert("RGB"))
    assert name == "im01.png" and x.device.type == "cuda"
    assert torch.equal(x, letterbox_u8_image(img, (48, 60), auto=True, scaleup=False, device=torch.device(DEV))[0])
    small = LowLightTestDataset(str(tmp_path), max_size=32)[1][0]
    assert torch.equal(small, letterbox_u8_image(img, 32, auto=True, scaleup=False, device=torch.device(DEV))[0])
    batches = list(get_test_dataloader(str(tmp_path), batch_size=2))
    assert [(tuple(b.shape), n) for b, n in batches] == [((2,) + tuple(x.shape), ["im00.png", "im01.png"]),
                                                         ((1,) + tuple(x.shape), ["im02.png"])]
    assert torch.equal(batches[0][0][1], x)


def test_letterbox_out_destination():
    from utils.letterbox import letterbox_shape, letterbox_u8_image
    img = np.random.default_rng(1).integers(0, 255, (50, 70, 3), dtype=np.uint8)
    want = letterbox_u8_image(img, 64, auto=True, scaleup=True, device=torch.device(DEV))[0]
    assert tuple(want.shape[1:]) == letterbox_shape((50, 70), 64, auto=True, scaleup=True)
    buf = torch.zeros((2,) + tuple(want.shape), device=DEV)
    got = letterbox_u8_image(img, 64, auto=True, scaleup=True, device=torch.device(DEV), out=buf[1])[0]
    assert got.data_ptr() == buf[1].data_ptr() and torch.equal(buf[1], want) and (buf[0] == 0).all()
    with pytest.raises(ValueError):
        letterbox_u8_image(img, 64, auto=True, scaleup=True, device=torch.device(DEV), out=buf[0, :, :-1])
