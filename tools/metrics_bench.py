#!/usr/bin/env python3
"""Image-quality metrics on the device (upr_image_metrics: utils/utils.py
calculate_metrics for a batch), timed with HIP events on the launching stream.

Two calls over a resident B x 3 x S x S fp32 batch: paired (enh + ground
truth: all nine metrics) and unpaired (the six no-reference metrics).  Four
copies of the inputs are cycled, so a call never finds its images in the 256 MB
last-level cache; the iteration count is set from a short probe so the timed
window is about --seconds.  Reported per call: ms, images/s, the algorithmic
bytes (each input image read once; the fp64 tile partials are < 0.5 % of that)
over time as a share of the 8 TB/s HBM peak, and fp64 operations per second
from the kernel's own operation count (ops_per_pixel below: one per fp64 add,
subtract, multiply, divide or square root the code performs, border tiles
counted like interior ones; the halo rows of the 16 x 32 tiles are included).

The baseline is the CPU restatement of the same arithmetic (tests/metrics_ref.py,
numpy float64) over the same images on --cpu-procs worker processes; it runs
before the device is touched.  It is a restatement, not the reference's scipy
code, and is labelled as such.

  python tools/metrics_bench.py [--batch 32] [--size 512] [--out profiles/metrics_bench_v1.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "retinex-image-enhancement_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402

PEAK_HBM_GBS = 8000.0
# csrc/metrics.hip's tile geometry
TH, TW, HALO, NQ = 16, 32, 5, 3


def ops_per_pixel(paired):
    """fp64 operations of metrics_tile_kernel per tile pixel, counted from its code."""
    px = TH * TW
    point = 3 * 3 + 1 + (3 * 3 if paired else 0)           # sums, squares, saturation (, squared error)
    niqe_rows = (TH + 2 * NQ) * (TW // 4) * (2 * 6 + 3 * 4)  # first of 4: 6 adds x 2; 3 slides x 2 ops x 2
    niqe_cols = px // 2 * (2 * 7 + 4 + 2 * 7)              # per thread: 7 adds x 2, one slide, 2 outputs x 7
    ssim = 0
    if paired:
        rows = (TH + 2 * HALO) * (TW // 4) * (3 + 10 * 8 + 3 * 16)  # products + 5 sums; 3 slides of 5 sums
        cols = px // 2 * (5 * (11 + 2) + 2 * 20)                     # 5 column sums with one slide; 2 quotients
        ssim = 3 * (rows + cols)
    return point + (niqe_rows + niqe_cols + ssim) / px


def make_images(B, S, copies):
    out = []
    for k in range(copies):
        rng = np.random.default_rng(100 + k)
        gt = rng.random((B, 3, S, S), dtype=np.float32)
        enh = np.clip(gt + np.float32(0.1) * (rng.random((B, 3, S, S), dtype=np.float32) - np.float32(0.5)), 0, 1)
        out.append((enh.astype(np.float32), gt))
    return out


def _cpu_one(args):
    import metrics_ref
    x, g = args
    return metrics_ref.metrics(x, g)[0]


def cpu_baseline(enh, gt, procs):
    """Seconds for the numpy restatement over the batch on `procs` processes: (paired, unpaired)."""
    import multiprocessing as mp
    res = {}
    with mp.get_context("fork").Pool(procs) as pool:
        pool.map(_cpu_one, [(enh[0], gt[0])] * procs)  # start the workers, import numpy
        for name, items in (("paired", [(x, g) for x, g in zip(enh, gt)]), ("unpaired", [(x, None) for x in enh])):
            t0 = time.perf_counter()
            out = pool.map(_cpu_one, items, chunksize=1)
            res[name] = (time.perf_counter() - t0, np.stack(out))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=0, help="fixed iteration count (0: from a probe)")
    ap.add_argument("--cpu-procs", type=int, default=16, help="0 skips the CPU baseline")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    B, S = args.batch, args.size
    imgs = make_images(B, S, args.copies)
    cpu = cpu_baseline(imgs[0][0], imgs[0][1], args.cpu_procs) if args.cpu_procs > 0 else None

    import torch
    from upr import runtime
    if not torch.cuda.is_available():
        sys.exit("metrics_bench needs a ROCm device")
    dev = torch.device("cuda", 0)
    bufs = [(torch.from_numpy(e).to(dev), torch.from_numpy(g).to(dev)) for e, g in imgs]
    px = B * S * S
    result = {"what": "image_metrics", "batch": B, "size": S, "dtype": "fp32", "input_copies_cycled": args.copies,
              "tile": [TH, TW], "peak_hbm_GBs": PEAK_HBM_GBS, "calls": {}}

    def timed(fn, iters):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    for name, paired in (("paired", True), ("unpaired", False)):
        def fn(i):
            e, g = bufs[i % len(bufs)]
            return runtime.image_metrics(e, g if paired else None)
        for i in range(2 * len(bufs)):
            fn(i)  # warm-up: code objects, the workspace
        probe = timed(fn, 2 * len(bufs))
        iters = args.iters or max(len(bufs), int(args.seconds * 1e3 / probe))
        ms = timed(fn, iters)
        got = fn(0)[0].cpu().numpy()
        nbytes = (24.0 if paired else 12.0) * px
        ops = ops_per_pixel(paired) * px
        rec = {"iters": iters, "timed_window_s": ms * iters / 1e3, "ms_per_call": ms, "images_per_s": B / ms * 1e3,
               "alg_bytes": nbytes, "achieved_GBs": nbytes / ms / 1e6, "frac_hbm": nbytes / ms / 1e6 / PEAK_HBM_GBS,
               "hbm_floor_ms": nbytes / PEAK_HBM_GBS / 1e6, "fp64_ops_per_px": ops_per_pixel(paired),
               "fp64_Gops_per_s": ops / ms / 1e6}
        if cpu is not None:
            sec, want = cpu[name]
            k = 9 if paired else 6
            rec["baseline"] = {"what": f"CPU restatement (tests/metrics_ref.py, numpy float64), {args.cpu_procs} "
                                       f"processes, the same {B} images", "ms_per_call": sec * 1e3,
                               "images_per_s": B / sec, "speedup": sec * 1e3 / ms,
                               "max_rel_diff_vs_device": float(np.max(np.abs(got[:, :k] - want[:, :k]) /
                                                                      np.abs(want[:, :k])))}
        result["calls"][name] = rec
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
