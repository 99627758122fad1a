#!/usr/bin/env python3
"""Illumination-weighted non-local means (upr.denoise.nlm): op time against a counted floor,
and what --denoise nlm costs the directory harness.

  python tools/denoise_bench.py [--rounds 10] [--harness_rounds 3] [--out profiles/denoise_v1.json]

Op time: 8 x and 32 x 512^2 images, (search, patch) = (5, 2) and (3, 1), on the harness bench's
noisy images (tools/harness_bench.py write_inputs) and on the real crop of
tests/golden/g4_real_crop.npz tiled (tools/png_bench.py); the map is the image's channel mean as
a u8 [B,H,W,3] tensor, as the harness passes it.  One call between device events per
configuration and round, the configurations alternating inside a round; medians over --rounds
after a warm-up of every configuration.

Floors, counted, not measured: the 32-bit vector integer instructions of the separable form the
kernel implements (int_ops_per_pixel) at the part's vector integer issue rate, 256 CUs x 4 SIMDs x
32 lanes x 2.4 GHz = 78.6 T instructions/s; and 3 B read + 1 B of map + 3 B written per pixel over
6.29 TB/s, the copy rate measured for this part (upr.calib's rate of this run is recorded
beside it).  The LDS reads (1 + 2P / 8 pixel reads and one weight lookup per pixel and offset)
go to the LDS pipe and are not in the count.

Harness: tools/harness_bench.py run() on one directory of 32 noisy 512^2 PNGs, denoise off
and nlm alternating, --harness_rounds times each after one uncounted round: images/s as median
and range, for the host and the device PNG encoder at batch 32.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "retinex-image-enhancement_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import harness_bench  # noqa: E402
from png_bench import real_images  # noqa: E402

HBM_TBPS = 6.29
INT_TOPS = 256 * 4 * 32 * 2.4e9 / 1e12
ROWS_PER_WAVE = 8  # csrc/denoise.hip kRows


def int_ops_per_pixel(search, patch):
    """Vector integer instructions per output pixel of the kernel's separable form."""
    per_offset = ((1 + 2 * patch / ROWS_PER_WAVE) * 3  # squared difference: one packed dot product, two adds
                  + 2                                   # the column sum slides one row: an add and a subtract
                  + 4 * patch                           # the 2P neighbouring columns' sums: 2P lane moves, 2P adds
                  + 4 + 1                               # t: the low 32 x 32 product (quarter rate) and its shift
                  + 3                                   # d <= dmax and the candidate inside the rectangle; the index
                  + 7)                                  # three channels unpacked, three multiply-adds, the weight sum
    return (2 * search + 1) ** 2 * per_offset * 64 / (64 - 2 * patch)  # 2P of a wave's 64 columns are halo


def noisy_images(n, size):
    rng = np.random.default_rng(0)
    return (rng.integers(0, 256, (n, size, size, 3)) * 0.35).astype(np.uint8)


def op_times(rounds):
    from upr import denoise
    configs = []
    for n in (8, 32):
        for name, imgs in (("noisy", noisy_images(n, 512)), ("real_crop_tiled", real_images(n, 512))):
            x = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
            m = x.float().mean(3, keepdim=True).round().to(torch.uint8).expand(-1, -1, -1, 3).contiguous()
            out = torch.empty_like(x)
            for search, patch in ((5, 2), (3, 1)):
                configs.append(dict(images=n, size=512, data=name, search=search, patch=patch, x=x, m=m, out=out,
                                    ms=[]))
    for c in configs:  # warm-up: code objects, allocator
        for _ in range(3):
            denoise.nlm(c["x"], c["m"], None, 1.0, 16, c["search"], c["patch"], out=c["out"])
    torch.cuda.synchronize()
    for _ in range(rounds):
        for c in configs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            denoise.nlm(c["x"], c["m"], None, 1.0, 16, c["search"], c["patch"], out=c["out"])
            e1.record()
            e1.synchronize()
            c["ms"].append(e0.elapsed_time(e1))
    res = []
    for c in configs:
        npix = c["images"] * c["size"] * c["size"]
        ops = int_ops_per_pixel(c["search"], c["patch"])
        int_floor = npix * ops / (INT_TOPS * 1e12) * 1e3
        hbm_floor = npix * 7 / (HBM_TBPS * 1e12) * 1e3
        med = statistics.median(c["ms"])
        res.append({k: c[k] for k in ("images", "size", "data", "search", "patch")} |
                   {"ms_median": med, "ms_min": min(c["ms"]), "ms_max": max(c["ms"]), "rounds": rounds,
                    "Mpixels_per_s": npix / med / 1e3, "int_ops_per_pixel": ops, "int_floor_ms": int_floor,
                    "share_of_int_floor": int_floor / med, "hbm_floor_ms": hbm_floor,
                    "bound_by": "vector integer issue" if int_floor > hbm_floor else "HBM"})
    return res


def harness(rounds):
    res = []
    with tempfile.TemporaryDirectory(dir="/tmp") as d:
        src = os.path.join(d, "in")
        harness_bench.write_inputs(src, 32, 512)
        for encoder in ("host", "device"):
            rates = {"off": [], "nlm": []}
            for rnd in range(rounds + 1):  # round 0 warms both and is not counted
                for mode in rates:
                    r = harness_bench.run(src, os.path.join(d, f"out_{encoder}_{mode}{rnd}"), 32, 512,
                                          png_encoder=encoder, batch_size=32, warm=False, denoise=mode)
                    assert r["files_written"] == 96, r
                    if rnd:
                        rates[mode].append(r["value"])
            row = {"png_encoder": encoder, "batch_size": 32, "n": 32, "size": 512, "rounds": rounds,
                   "unit": "images/s"}
            for mode, v in rates.items():
                row[mode] = {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}
            row["nlm_over_off"] = row["nlm"]["median"] / row["off"]["median"]
            res.append(row)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--harness_rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("denoise_bench needs a ROCm device")
    from upr import calib
    res = {"metric": "illumination-weighted non-local means (upr.denoise.nlm), device-event time per call, and the "
                     "directory harness with --denoise off / nlm",
           "int_Tops_for_floors": INT_TOPS, "hbm_TBps_for_floors": HBM_TBPS,
           "hbm_copy_TBps_this_run": calib.measure(torch.device("cuda"), warm_s=0.5)["hbm_copy_TBps"],
           "op": op_times(args.rounds)}
    if args.harness_rounds > 0:
        res["harness"] = harness(args.harness_rounds)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
