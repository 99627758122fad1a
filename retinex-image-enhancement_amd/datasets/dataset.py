"""Low-light image datasets and loaders (drop-in for the reference
datasets/dataset.py; same names and signatures).

The reference augments every sample on a DataLoader worker process with torch
CPU ops.  Here a worker THREAD only PIL-decodes to uint8 HWC; everything after
the decode runs on the device, on the main thread's stream: the bytes are
uploaded, letterboxed into the sample's slot of the batch buffer
(utils.letterbox.letterbox_u8_image, out=), and one upr.augment.augment call
applies the flips, rot90 and the photometric chain to the whole batch.  No
process is forked and no worker touches the GPU.

`draw_params` consumes Python's `random` exactly as the reference's
__getitem__ / _apply_advanced_augmentation do (dataset.py:104-114, :133-161),
so one `random.seed` gives the same decisions and values as the reference run
with num_workers=0.  The noise itself is the device generator's (Philox keyed
by the loader's seed and the sample id = epoch * len(dataset) + index), not
torch.randn_like's.
"""
import os
import random
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

from upr import augment as uaug
from utils.letterbox import letterbox_shape, letterbox_u8_image

VALID_EXTENSIONS = {'.jpg', '.jpeg', '.png', '.bmp'}
MAX_DECODE_THREADS = 16


def draw_params(augment=True, advanced_augment=True, rng=random):
    """One sample's augmentation draw -> dict(hflip, vflip, k, gamma, contrast,
    brightness, noise_level, saturation, shift); a photometric stage that did
    not fire is None.  rng: the `random` module or a random.Random."""
    p = {"hflip": False, "vflip": False, "k": 0, "gamma": None, "contrast": None, "brightness": None,
         "noise_level": None, "saturation": None, "shift": None}
    if augment:
        p["hflip"] = rng.random() > 0.5
        p["vflip"] = rng.random() > 0.5
        if rng.random() > 0.5:
            p["k"] = rng.choice([1, 2, 3])
    if advanced_augment:
        if rng.random() > 0.5:
            p["gamma"] = rng.uniform(0.6, 1.8)
        if rng.random() > 0.5:
            p["contrast"] = rng.uniform(0.8, 1.2)
        if rng.random() > 0.5:
            p["brightness"] = rng.uniform(-0.1, 0.1)
        if rng.random() > 0.3:
            p["noise_level"] = rng.uniform(0.01, 0.03)
        if rng.random() > 0.5:
            p["saturation"] = rng.uniform(0.8, 1.2)
        if rng.random() > 0.5:
            p["shift"] = rng.uniform(-0.05, 0.05)
    return p


def _list_images(image_dir):
    files = []
    for root, _, names in os.walk(image_dir):
        files += [os.path.join(root, n) for n in names if os.path.splitext(n)[1].lower() in VALID_EXTENSIONS]
    return sorted(files)


def match_by_stem(files, reference_files, reference_dir):
    """The ground truth of every NAME.ext of `files`: the file of reference_files
    with stem NAME (the first in sorted order when several share it), in the
    order of `files`.  A file without one raises ValueError naming it."""
    by_stem = {}
    for f in reference_files:
        by_stem.setdefault(os.path.splitext(os.path.basename(f))[0], f)
    stems = [os.path.splitext(os.path.basename(f))[0] for f in files]
    missing = [f for f, st in zip(files, stems) if st not in by_stem]
    if missing:
        raise ValueError(f"no ground truth in '{reference_dir}' for {', '.join(repr(m) for m in missing)} "
                         f"(matched by file stem)")
    return [by_stem[st] for st in stems]


def decode_u8(path):
    """PIL decode -> uint8 [H,W,3] (the only per-sample work left on the host)."""
    return np.array(Image.open(path).convert('RGB'), dtype=np.uint8)


def _default_device(device):
    if not torch.cuda.is_available():
        raise RuntimeError("the training data path runs on ROCm devices only (no CPU fallback)")
    dev = torch.device(device) if device is not None else torch.device("cuda")
    if dev.type != "cuda":
        raise RuntimeError(f"the training data path runs on ROCm devices only, not on {dev}")
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


class LowLightDataset:
    """Reference dataset.py:21-183.  `device` and `seed` (the noise generator's
    key) are attributes, set by the loader or by hand; random_crop is accepted
    and unused, as in the reference."""

    def __init__(self, image_dir, image_size=640, random_crop=True, augment=True, advanced_augment=True):
        self.image_dir = image_dir
        self.image_size = image_size
        self.random_crop = random_crop
        self.augment = augment
        self.advanced_augment = advanced_augment
        self.device = None
        self.seed = 0
        self.image_files = _list_images(image_dir)
        if len(self.image_files) == 0:
            raise ValueError(f"No images found in {image_dir}")
        print(f"Loaded {len(self.image_files)} images from {image_dir}")

    def __len__(self):
        return len(self.image_files)

    def letterboxed(self, img_u8, device, out=None):
        """dataset.py:91-99: ToTensor + letterbox_tensor(new_shape=image_size, auto, scaleup) on the device."""
        return letterbox_u8_image(img_u8, self.image_size, auto=True, scaleup=True, device=device, out=out)[0]

    def __getitem__(self, idx):
        """One augmented [3,H,W] device tensor: a batch-of-one augment call, drawn from the global `random`."""
        dev = _default_device(self.device)
        x = self.letterboxed(decode_u8(self.image_files[idx]), dev)
        p = draw_params(self.augment, self.advanced_augment)
        return uaug.augment(x[None], uaug.pack([p], [idx]), seed=self.seed)[0]


class PairedLowLightDataset(LowLightDataset):
    """Low-light images with their ground truth (an addition: the reference
    trains without labels).  reference_files[i] is the file of reference_dir
    whose stem is that of image_files[i] (match_by_stem).  An item is (low,
    target): both letterboxed the same way, the target given the sample's flips
    and rot90 and none of its photometric stages."""

    def __init__(self, image_dir, reference_dir, image_size=640, random_crop=True, augment=True,
                 advanced_augment=True):
        super().__init__(image_dir, image_size=image_size, random_crop=random_crop, augment=augment,
                         advanced_augment=advanced_augment)
        self.reference_dir = reference_dir
        self.reference_files = match_by_stem(self.image_files, _list_images(reference_dir), reference_dir)

    def __getitem__(self, idx):
        dev = _default_device(self.device)
        low, gt = decode_pair(self.image_files[idx], self.reference_files[idx])
        x, y = self.letterboxed(low, dev), self.letterboxed(gt, dev)
        p = draw_params(self.augment, self.advanced_augment)
        return (uaug.augment(x[None], uaug.pack([p], [idx]), seed=self.seed)[0],
                uaug.augment(y[None], uaug.target_records([p], [idx]), seed=self.seed)[0])


def check_pair(low, gt, low_file, gt_file):
    """A pair whose decoded sizes differ is refused, naming the two files."""
    if low.shape != gt.shape:
        raise ValueError(f"'{low_file}' decodes to {low.shape[1]}x{low.shape[0]} and its ground truth '{gt_file}' to "
                         f"{gt.shape[1]}x{gt.shape[0]}: a pair must have one size")


def decode_pair(low_file, gt_file):
    low, gt = decode_u8(low_file), decode_u8(gt_file)
    check_pair(low, gt, low_file, gt_file)
    return low, gt


class LowLightTestDataset:
    """Reference dataset.py:186-258: no augmentation; (image [3,H,W] on the device, file name)."""

    def __init__(self, image_dir, max_size=None):
        self.image_dir = image_dir
        self.max_size = max_size
        self.device = None
        self.image_files = _list_images(image_dir)
        if len(self.image_files) == 0:
            raise ValueError(f"No images found in {image_dir}")
        print(f"Loaded {len(self.image_files)} test images from {image_dir}")

    def __len__(self):
        return len(self.image_files)

    def __getitem__(self, idx):
        path = self.image_files[idx]
        img = decode_u8(path)
        new_shape = self.max_size if self.max_size is not None else img.shape[:2]
        x, _, _ = letterbox_u8_image(img, new_shape, auto=True, scaleup=False, device=_default_device(self.device))
        return x, os.path.basename(path)


class DeviceLoader:
    """Batches of a LowLightDataset as [B,3,H,W] float32 device tensors; of a
    PairedLowLightDataset as (low, target) pairs of them: both files go through
    the decode threads and the same letterbox, the target through a second
    augment call whose records carry the sample's geometry alone
    (upr.augment.target_records), and the parameter draws are those of the
    unpaired loader.

    min(num_workers, 16) threads decode ahead (0: decode inline); the main
    thread uploads, letterboxes, draws the parameters in sample order and makes
    one augment call per batch.  Two batches are kept in flight: batch n+1 is
    queued on the stream before batch n is handed out.  With a seed, the shuffle
    and the parameter draws come from generators seeded by (seed, epoch) and the
    noise from (seed, sample id), so an epoch is reproducible whatever the batch
    size; without one, the draws come from the global `random` (the reference's
    source).  The epoch advances by one per iteration; set_epoch overrides it."""

    def __init__(self, dataset, batch_size=8, shuffle=True, num_workers=4, drop_last=False, device=None, seed=None):
        self.dataset = dataset
        self.batch_size = int(batch_size)
        self.shuffle = shuffle
        self.num_workers = max(0, min(int(num_workers), MAX_DECODE_THREADS))
        self.drop_last = drop_last
        self.device = device
        self.seed = seed
        self.noise_seed = int(seed) if seed is not None else random.getrandbits(63)
        self.epoch = 0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def _order(self, epoch):
        order = list(range(len(self.dataset)))
        if self.shuffle:
            rng = random.Random(self.seed * 1000003 + epoch) if self.seed is not None else random
            rng.shuffle(order)
        return order

    def _plan(self, epoch):
        """(the epoch's batches of sample indices, the generator of its parameter draws)."""
        order = self._order(epoch)
        bs = self.batch_size
        batches = [order[i:i + bs] for i in range(0, len(order), bs)]
        if self.drop_last and batches and len(batches[-1]) < bs:
            batches.pop()
        rng = random.Random(self.seed * 1000003 + epoch + 500009) if self.seed is not None else random
        return batches, rng

    def _draw(self, count, rng):
        """One batch's draws, in sample order."""
        ds = self.dataset
        return [draw_params(ds.augment, ds.advanced_augment, rng) for _ in range(count)]

    def _assemble(self, idxs, images, epoch, rng, dev, targets=None):
        ds = self.dataset
        files = [ds.image_files[i] for i in idxs]
        if targets is not None:
            for i, im, gt in zip(idxs, images, targets):
                check_pair(im, gt, ds.image_files[i], ds.reference_files[i])
        shapes = [letterbox_shape(im.shape[:2], ds.image_size, auto=True, scaleup=True) for im in images]
        if any(s != shapes[0] for s in shapes):
            raise RuntimeError("images of one batch letterbox to different shapes: " +
                               ", ".join(f"{f} {s}" for f, s in zip(files, shapes)))
        H, W = shapes[0]
        x = torch.empty((len(idxs), 3, H, W), dtype=torch.float32, device=dev)
        for slot, im in enumerate(images):
            ds.letterboxed(im, dev, out=x[slot])
        params = self._draw(len(images), rng)
        if H != W and len({p["k"] & 1 for p in params}) > 1:
            raise RuntimeError("rot90 gives the images of one batch different shapes: " +
                               ", ".join(f"{f} k={p['k']}" for f, p in zip(files, params)))
        ids = [epoch * len(ds) + i for i in idxs]
        low = uaug.augment(x, uaug.pack(params, ids), seed=self.noise_seed)
        if targets is None:
            return low
        y = torch.empty_like(x)
        for slot, gt in enumerate(targets):
            ds.letterboxed(gt, dev, out=y[slot])
        return low, uaug.augment(y, uaug.target_records(params, ids), seed=self.noise_seed)

    def __iter__(self):
        epoch = self.epoch
        self.epoch += 1
        dev = _default_device(self.device if self.device is not None else self.dataset.device)
        batches, rng = self._plan(epoch)
        files = self.dataset.image_files
        # a paired dataset: the ground truth of a batch is decoded behind its low-light files, by the same threads
        gts = getattr(self.dataset, "reference_files", None)
        pool = ThreadPoolExecutor(max_workers=self.num_workers) if self.num_workers else None
        try:
            todo, decoding, ready = iter(batches), deque(), deque()

            def decode_ahead():  # the threads work up to two batches ahead of the assembly
                while len(decoding) < 2:
                    idxs = next(todo, None)
                    if idxs is None:
                        return
                    paths = [files[i] for i in idxs] + ([gts[i] for i in idxs] if gts is not None else [])
                    decoding.append((idxs, [pool.submit(decode_u8, f) for f in paths] if pool else None, paths))

            decode_ahead()
            while decoding or ready:
                while decoding and len(ready) < 2:
                    idxs, futs, paths = decoding.popleft()
                    decode_ahead()
                    images = [f.result() for f in futs] if futs else [decode_u8(f) for f in paths]
                    n = len(idxs)
                    ready.append(self._assemble(idxs, images[:n], epoch, rng, dev, images[n:] if gts is not None
                                                else None))
                yield ready.popleft()
        finally:
            if pool is not None:
                pool.shutdown(wait=True, cancel_futures=True)


def get_train_dataloader(image_dir, batch_size=8, image_size=640, num_workers=4, shuffle=True,
                         advanced_augment=False, drop_last=False, *, device=None, seed=None, reference_dir=None):
    """Reference dataset.py:261-300 (augment=True always), plus device= and seed=;
    reference_dir= makes it a paired loader of (low, target) batches."""
    if reference_dir is not None:
        dataset = PairedLowLightDataset(image_dir, reference_dir, image_size=image_size, random_crop=True,
                                        augment=True, advanced_augment=advanced_augment)
    else:
        dataset = LowLightDataset(image_dir=image_dir, image_size=image_size, random_crop=True, augment=True,
                                  advanced_augment=advanced_augment)
    dataset.device = device
    if seed is not None:
        dataset.seed = int(seed)
    return DeviceLoader(dataset, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers,
                        drop_last=drop_last, device=device, seed=seed)


class _TestLoader:
    """Sequential (images [B,3,H,W], names) batches of a LowLightTestDataset."""

    def __init__(self, dataset, batch_size):
        self.dataset = dataset
        self.batch_size = int(batch_size)

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        for i in range(0, len(self.dataset), self.batch_size):
            items = [self.dataset[j] for j in range(i, min(i + self.batch_size, len(self.dataset)))]
            if any(x.shape != items[0][0].shape for x, _ in items):
                raise RuntimeError("images of one batch differ in shape: " + ", ".join(n for _, n in items))
            yield torch.stack([x for x, _ in items]), [n for _, n in items]


def get_test_dataloader(image_dir, batch_size=1, max_size=None, num_workers=2):
    """Reference dataset.py:303-332; num_workers is accepted for the signature (the decode is inline)."""
    return _TestLoader(LowLightTestDataset(image_dir=image_dir, max_size=max_size), batch_size)
