#!/usr/bin/env python3
"""Golden vectors of the reference's photometric augmentation (run ONCE in the
build container, never on the GPU box).

Imports the reference datasets/dataset.py read-only and records what
LowLightDataset._apply_advanced_augmentation / _adjust_saturation compute on
seeded inputs.  The reference module imports cv2 and torchvision, which are not
installed here and which these two methods never touch: empty stand-in modules
are registered so the import succeeds, and the methods run on an instance made
without __init__.  Only arrays are written; no reference source is copied.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_augment.py

For every seed s: random.seed(s); torch.manual_seed(s); the method on the fp32
input -> out32.  The one torch.randn_like draw the method makes is re-derived
(manual_seed(s); torch.randn(shape)) and injected into a second call on the
float64 copy of the input -> out64.  ref_err = max |out32 - out64| over all
cases: the reference's own fp32 rounding, the unit of the GPU test's bound.

Files (each below the 1 MiB limit for a committed file, hence the parts):
  g9_augment.npz           index: shapes, seeds, the two inputs per shape
                           (plain, and scaled by 0.3 for odd seeds), ref_err,
                           and the cases of the second shape
  g9_augment_s<first>.npz  the 3 x 40 x 40 cases, PART seeds per file
Case arrays are named <shape>_<seed>_{noise,out32,out64}.
"""
import os
import random
import sys
import types

import numpy as np
import torch

REF = os.environ.get("UPR_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

for name in ("cv2", "torchvision", "torchvision.transforms"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]

from datasets import dataset as ref_ds  # noqa: E402  (reference datasets/dataset.py)

SHAPES = {"a": (3, 40, 40), "b": (3, 33, 47)}   # square with partial transpose tiles; W % 4 != 0
SEEDS = {"a": list(range(34)), "b": [0, 4, 5, 33]}  # 33: all six stages on, 4: all off
PART = 12


def run(ds, seed, x, noise=None):
    random.seed(seed)
    torch.manual_seed(seed)
    if noise is None:
        return ds._apply_advanced_augmentation(x)
    keep = torch.randn_like
    torch.randn_like = lambda t: noise.to(t.dtype)
    try:
        return ds._apply_advanced_augmentation(x)
    finally:
        torch.randn_like = keep


def main():
    ds = ref_ds.LowLightDataset.__new__(ref_ds.LowLightDataset)
    index = {"ref_err": 0.0}
    parts = {}
    ref_err = 0.0
    for key, shape in SHAPES.items():
        base = torch.rand(shape, generator=torch.Generator().manual_seed(1234 + shape[2]))
        inputs = torch.stack([base, base * 0.3])  # odd seeds take the low-light one
        index[f"{key}_inputs"] = inputs.numpy()
        index[f"{key}_seeds"] = np.asarray(SEEDS[key], np.int64)
        for s in SEEDS[key]:
            x = inputs[s % 2]
            out32 = run(ds, s, x)
            torch.manual_seed(s)
            noise = torch.randn(shape)
            assert torch.equal(run(ds, s, x, noise), out32), "the method draws more than one randn_like"
            out64 = run(ds, s, x.double(), noise)
            assert out32.dtype == torch.float32 and out64.dtype == torch.float64
            ref_err = max(ref_err, (out32.double() - out64).abs().max().item())
            dst = index if key == "b" else parts.setdefault(f"g9_augment_s{s // PART * PART:02d}.npz", {})
            dst[f"{key}_{s}_noise"] = noise.numpy()
            dst[f"{key}_{s}_out32"] = out32.numpy()
            dst[f"{key}_{s}_out64"] = out64.numpy()
    index["ref_err"] = np.float64(ref_err)
    index["parts"] = np.asarray(sorted(parts))
    np.savez_compressed(os.path.join(OUT, "g9_augment.npz"), **index)
    for name, arrays in parts.items():
        np.savez_compressed(os.path.join(OUT, name), **arrays)
    for name in ["g9_augment.npz"] + sorted(parts):
        print(name, os.path.getsize(os.path.join(OUT, name)), "bytes")
    print("ref_err", ref_err)


if __name__ == "__main__":
    main()
