#!/usr/bin/env python3
"""Device PNG encoder (upr.png): encode time, file size against PIL, bytes over the HBM rate.

Two sets of 32 images of 512 x 512: the harness bench's synthetic low-light noise
(tools/harness_bench.py) and the real crop of tests/golden/g4_real_crop.npz tiled to 512 x 512
(each image of the batch shifted by a few pixels so the files differ).

  python tools/png_bench.py [--n 32] [--size 512] [--reps 50] [--matches lz] [--out profiles/png_encode_v1.json]

--matches lz measures every set with matches="lz" and, in the same run, with matches="none".

Times are device events around upr.png.encode_device (its three kernels, no copy to the host),
median of --reps calls after a warm-up.  hbm_floor_ms is (pixels read + file bytes written) over
the copy rate upr.calib measures; the encoder reads the pixels more than once, so this is a floor
for the format, not for this implementation.
"""
import argparse
import io
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "retinex-image-enhancement_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402


def harness_images(n, size):
    rng = np.random.default_rng(0)
    return np.stack([(rng.integers(0, 256, (size, size, 3)) * 0.35).astype(np.uint8) for _ in range(n)])


def real_images(n, size):
    crop = np.load(os.path.join(REPO, "tests", "golden", "g4_real_crop.npz"))["img_u8"]
    reps = -(-size // crop.shape[0]), -(-size // crop.shape[1])
    tiled = np.tile(crop, (reps[0], reps[1], 1))[:size, :size]
    return np.stack([np.roll(tiled, (3 * k, 5 * k), (0, 1)) for k in range(n)])


def pil_bytes(a, **kw):
    f = io.BytesIO()
    Image.fromarray(a).save(f, format="PNG", **kw)
    return f.tell()


def measure_set(name, imgs, reps, hbm_TBps, filter, rows_per_strip, matches="none"):
    from upr import png
    x = torch.from_numpy(imgs).cuda()
    files = png.encode(x, filter=filter, rows_per_strip=rows_per_strip, matches=matches)
    for k in (0, len(files) - 1):  # the decoder is the check
        assert np.array_equal(np.array(Image.open(io.BytesIO(files[k]))), imgs[k]), (name, k)
    for _ in range(5):
        png.encode_device(x, filter=filter, rows_per_strip=rows_per_strip, matches=matches)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        png.encode_device(x, filter=filter, rows_per_strip=rows_per_strip, matches=matches)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    dev_bytes = sum(len(f) for f in files)
    sample = range(0, len(imgs), max(1, len(imgs) // 4))  # PIL on a few images is enough for a ratio
    pil_def = sum(pil_bytes(imgs[k]) for k in sample)
    pil_l1 = sum(pil_bytes(imgs[k], compress_level=1) for k in sample)
    dev_sample = sum(len(files[k]) for k in sample)
    moved = imgs.nbytes + dev_bytes
    floor_ms = moved / (hbm_TBps * 1e12) * 1e3
    med = statistics.median(ms)
    return {"set": name, "matches": matches, "images": int(imgs.shape[0]), "size": int(imgs.shape[1]),
            "filter": filter,
            "rows_per_strip": rows_per_strip, "encode_ms_median": med, "encode_ms_min": min(ms),
            "encode_ms_max": max(ms), "reps": reps, "images_per_s": imgs.shape[0] / (med * 1e-3),
            "pixel_bytes": int(imgs.nbytes), "device_file_bytes": int(dev_bytes),
            "device_bytes_per_image": dev_bytes / imgs.shape[0],
            "pil_default_bytes_per_image": pil_def / len(sample), "pil_level1_bytes_per_image": pil_l1 / len(sample),
            "device_over_pil_default": dev_sample / pil_def, "device_over_pil_level1": dev_sample / pil_l1,
            "device_over_raw": dev_bytes / imgs.nbytes, "hbm_floor_ms": floor_ms,
            "encode_ms_over_hbm_floor": med / floor_ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--filter", default="adaptive")
    ap.add_argument("--rows_per_strip", type=int, default=16)
    ap.add_argument("--matches", choices=["none", "lz"], default="none")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("png_bench needs a ROCm device")
    from upr import calib
    hbm = calib.measure(torch.device("cuda"), warm_s=0.5)["hbm_copy_TBps"]
    res = {"metric": "device PNG encode (upr.png.encode_device), device-event time per call",
           "hbm_copy_TBps": hbm,
           "sets": [measure_set(name, imgs, args.reps, hbm, args.filter, args.rows_per_strip, m)
                    for name, imgs in (("harness_noise", harness_images(args.n, args.size)),
                                       ("real_crop_tiled", real_images(args.n, args.size)))
                    for m in (("lz", "none") if args.matches == "lz" else ("none",))]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
