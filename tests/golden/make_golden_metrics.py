#!/usr/bin/env python3
"""Golden vectors of the reference's image-quality metrics (run ONCE on a host
that has the reference checkout and scipy, never on the GPU box).

Imports the reference's utils/utils.py read-only (UPR_REFERENCE names its root)
and records what calculate_metrics returns, with and without a ground truth, on
seeded inputs.  Only arrays are written; no reference source is copied.

    UPR_REFERENCE=<reference root> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_metrics.py

Shapes 8x8, 13x70, 37x53, 64x64, 96x160 (smaller than the 11-window, ragged,
several tiles).  Per shape, from np.random.default_rng(1000 + index), float32:
  gt  = 0.15 + 0.6 * ramp + 0.2 * noise   (ramp: per channel, a different mix of x / W and y / H)
  enh = clip(gt + 0.1 * (noise' - 0.5), 0, 1)
  low = 0.25 * gt
  q8  = floor(enh * 255) / 255
and for each of enh / low / q8 the reference's dict without and with gt.

tests/golden/g10_metrics.npz: <H>x<W>_gt, <H>x<W>_<kind>_x ([3,H,W] float32),
<H>x<W>_<kind>_unpaired / _paired (float64, the dict's values in its insertion
order, which the script checks against tests/metrics_ref.py's key lists).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import metrics_ref as R  # noqa: E402

REF = os.environ.get("UPR_REFERENCE")
if not REF:
    sys.exit("set UPR_REFERENCE to the root of the reference checkout")
# the reference's own `utils` package, not this repository's
sys.path.insert(0, REF)
for m in [k for k in sys.modules if k == "utils" or k.startswith("utils.")]:
    del sys.modules[m]
import matplotlib  # noqa: E402
matplotlib.use("Agg")
from utils import utils as ref_utils  # noqa: E402

assert os.path.abspath(ref_utils.__file__).startswith(os.path.abspath(REF))


def make_images(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float32) / h, np.arange(w, dtype=np.float32) / w, indexing="ij")
    mix = np.array([0.7, 0.5, 0.2], np.float32)
    ramp = np.stack([a * xx + (1 - a) * yy for a in mix]).astype(np.float32)
    noise = rng.random((3, h, w), dtype=np.float32)
    gt = (np.float32(0.15) + np.float32(0.6) * ramp + np.float32(0.2) * noise).astype(np.float32)
    noise2 = rng.random((3, h, w), dtype=np.float32)
    enh = np.clip(gt + np.float32(0.1) * (noise2 - np.float32(0.5)), 0, 1).astype(np.float32)
    low = (np.float32(0.25) * gt).astype(np.float32)
    q8 = (np.floor(enh * np.float32(255)) / np.float32(255)).astype(np.float32)
    return gt, {"enh": enh, "low": low, "q8": q8}


def main():
    import torch
    out = {}
    worst = {}
    for i, (h, w) in enumerate(R.SHAPES):
        gt, imgs = make_images(h, w, 1000 + i)
        out[f"{h}x{w}_gt"] = gt
        for kind in R.KINDS:
            x = imgs[kind]
            k = f"{h}x{w}_{kind}"
            out[f"{k}_x"] = x
            un = ref_utils.calculate_metrics(torch.from_numpy(x).unsqueeze(0))
            pa = ref_utils.calculate_metrics(torch.from_numpy(x).unsqueeze(0), torch.from_numpy(gt).unsqueeze(0))
            assert tuple(un) == R.UNPAIRED and tuple(pa) == R.PAIRED, (tuple(un), tuple(pa))
            assert all(np.isfinite(v) for v in pa.values()), (k, pa)
            out[f"{k}_unpaired"] = np.array([un[n] for n in R.UNPAIRED], np.float64)
            out[f"{k}_paired"] = np.array([pa[n] for n in R.PAIRED], np.float64)
            mine = R.metrics_dict(x, gt)
            for n in R.PAIRED:
                worst[n] = max(worst.get(n, 0.0), R.rel(mine[n], pa[n]))
    path = os.path.join(HERE, "g10_metrics.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
    print("restatement vs reference, worst relative difference per metric:")
    for n, v in worst.items():
        print(f"  {n:16s} {v:.2e}")


if __name__ == "__main__":
    main()
