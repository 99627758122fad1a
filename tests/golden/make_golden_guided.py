#!/usr/bin/env python3
"""Golden vectors for the guided-filter restore tests (run ONCE on a host that
has the reference checkout, never on the GPU box).

Imports the reference's models/model.py read-only (UPR_REFERENCE names its
root) and records what its UP_Retinex (seed 0, plain blocks, eval(): the model
of g4_real_crop.npz) returns on the letterboxed g4 crop: oracle.letterbox of
g4's img_u8 at max_size 64 (a 64 x 64 image, no bars).  Only arrays are
written; no reference source is copied.

    UPR_REFERENCE=<reference root> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_guided.py

tests/golden/g11_guided.npz: low_u8 (u8 [64,64,3], the letterboxed input), enh
([1,3,64,64] float32) and illu ([1,1,64,64] float32).  The full-resolution
yardstick is g4's own enh.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
from oracle import letterbox as olb  # noqa: E402

REF = os.environ.get("UPR_REFERENCE")
if not REF:
    sys.exit("set UPR_REFERENCE to the root of the reference checkout")
sys.path.insert(0, REF)
from models import model as ref_model  # noqa: E402  (reference models/model.py)

assert os.path.abspath(ref_model.__file__).startswith(os.path.abspath(REF))


def main():
    g4 = np.load(os.path.join(HERE, "g4_real_crop.npz"))
    low, _, _ = olb.letterbox(g4["img_u8"], new_shape=64, auto=True, scaleup=False)
    assert low.shape == (64, 64, 3)
    x = torch.from_numpy(low.astype(np.float32) / 255.0).permute(2, 0, 1).unsqueeze(0).contiguous()
    torch.manual_seed(0)
    m = ref_model.UP_Retinex(use_preact=False, use_aspp=False).eval()
    with torch.no_grad():
        e, _, i = m(x)
    path = os.path.join(HERE, "g11_guided.npz")
    np.savez_compressed(path, low_u8=low, enh=e.numpy(), illu=i.numpy())
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
