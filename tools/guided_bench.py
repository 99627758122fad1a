#!/usr/bin/env python3
"""Guided-filter restore (upr.guided): fit and apply times against their HBM floors, and,
with --quality_image, the restored output against the native full-size forward.

  python tools/guided_bench.py [--reps 30] [--out profiles/guided_v1.json] [--quality [--quality_image photo.jpg]]

Two workloads, sources from the real crop of tests/golden/g4_real_crop.npz tiled (tools/png_bench.py):
32 x (512^2 -> 1024^2) and 8 x (512^2 -> 2048^2).  The letterboxed side is the harness's own
(letterbox_u8_batch at max_size 512 on the staged sources); the target is a gamma curve of it and the
illumination map its channel mean, so no model runs.  Times are device events around one call
(fit: its two kernels; apply: its one), median of --reps after a warm-up.

Floors: bytes over 6.29 TB/s, the copy rate measured for this part (the README quotes letterbox and
panel pack the same way); upr.calib's rate of this run is recorded beside it.  apply moves 3 B read
plus 6 (enhanced + illumination), 12 (+ 2-panel comparison) or 15 (+ 3-panel) B written per source
pixel.  fit's floor is the operator's, 6 B read and 48 B written per content pixel; the two-kernel
form also writes and reads the 48 B a, b scratch.

--quality: one image (--quality_image, or without it the real crop of g4_real_crop.npz tiled to
1024 x 1024) -> PSNR (utils.batch_metrics) of the enhanced output restored from
--max_size 512 against the same model's forward at the photo's own size, with and without the CLAHE
step, and of plain bilinear upsampling of the letterboxed result (A = 0, B = target) for scale.
The model is UP_Retinex() at seed 0, random weights: the operator's fidelity, not a trained model's.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "retinex-image-enhancement_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from png_bench import real_images  # noqa: E402

HBM_TBPS = 6.29


def event_ms(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def stats(ms, floor_ms):
    med = statistics.median(ms)
    return {"ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "hbm_floor_ms": floor_ms,
            "share_of_hbm_floor": floor_ms / med}


def measure(n, size, max_size, reps, radius, eps):
    from upr import guided, runtime
    from utils.letterbox import letterbox_content, letterbox_u8_batch
    imgs = real_images(n, size)
    x, sources = letterbox_u8_batch(list(imgs), max_size, auto=True, scaleup=False, device="cuda",
                                    return_sources=True)
    content = letterbox_content((size, size), max_size, auto=True, scaleup=False)
    guide, illu, _ = runtime.panels_u8(x, x, x.mean(1, keepdim=True), None)
    target = runtime.panels_u8(x, x.pow(0.6).clamp(0, 1), None, None)[0]
    ab = guided.fit(guide, target, content, radius, eps)
    torch.cuda.synchronize()
    npix, ncontent = n * size * size, n * content[2] * content[3]
    res = {"images": n, "source_size": size, "max_size": max_size, "content": list(content), "radius": radius,
           "eps": eps, "reps": reps}
    res["fit"] = stats(event_ms(lambda: guided.fit(guide, target, content, radius, eps), reps),
                       ncontent * (6 + 48) / (HBM_TBPS * 1e12) * 1e3)
    for comparison, written in ((None, 6), (2, 12), (3, 15)):
        ms = event_ms(lambda: guided.apply(sources, ab, illu, content, comparison), reps)
        res[f"apply_{written}B_written"] = dict(stats(ms, npix * (3 + written) / (HBM_TBPS * 1e12) * 1e3),
                                                comparison=comparison, bytes_per_pixel=3 + written)
    return res


def _chw(u8):
    return u8.permute(0, 3, 1, 2).float() / 255.0


def quality(path, max_size, radius, eps):
    from PIL import Image
    from enhancers.adaptive_params import AdaptiveParameterAdjuster
    from models.model import UP_Retinex
    from upr import guided, runtime
    from utils.letterbox import letterbox_content, letterbox_u8_batch
    from utils.utils import batch_metrics
    if path is None:
        a = np.ascontiguousarray(real_images(1, 1024)[0])
    else:
        a = np.array(Image.open(path).convert("RGB"), dtype=np.uint8)
    H, W = a.shape[:2]
    torch.manual_seed(0)
    model = UP_Retinex().to("cuda").eval()
    out = {"image": os.path.basename(path) if path else "g4_real_crop.npz img_u8 tiled to 1024 x 1024",
           "source_size": [H, W], "max_size": max_size, "radius": radius, "eps": eps,
           "model": "UP_Retinex() preact + ASPP, seed 0 (random weights)"}
    x_full = letterbox_u8_batch([a], (H, W), auto=True, scaleup=False, device="cuda")
    x_low, sources = letterbox_u8_batch([a], max_size, auto=True, scaleup=False, device="cuda", return_sources=True)
    full_rect = letterbox_content((H, W), (H, W), auto=True, scaleup=False)
    rect = letterbox_content((H, W), max_size, auto=True, scaleup=False)
    out["letterboxed"], out["content"] = list(x_low.shape[2:]), list(rect)
    with torch.no_grad():
        e_full, e_low = model(x_full)[0], model(x_low)[0]
    clahe = AdaptiveParameterAdjuster().apply_clahe_enhancement
    for name, post in (("forward_only", lambda t: t), ("forward_and_clahe", clahe)):
        native = runtime.panels_u8(x_full, post(e_full), None, None)[0]
        t, l, nh, nw = full_rect
        native = native[:, t:t + nh, l:l + nw].contiguous()
        guide = runtime.panels_u8(x_low, x_low, None, None)[0]
        target = runtime.panels_u8(x_low, post(e_low), None, None)[0]
        restored = guided.restore(sources, guide, target, None, rect, radius, eps)[0]
        ab0 = torch.zeros((1, 2, 3, rect[2], rect[3]), dtype=torch.float64, device="cuda")
        ab0[:, 1] = target[:, rect[0]:rect[0] + rect[2], rect[1]:rect[1] + rect[3]].permute(0, 3, 1, 2).double()
        bilinear = guided.apply(sources, ab0)[0]
        out[name] = {"guided_psnr_db": float(batch_metrics(_chw(restored), _chw(native))["psnr"][0]),
                     "bilinear_psnr_db": float(batch_metrics(_chw(bilinear), _chw(native))["psnr"][0])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--max_size", type=int, default=512)
    ap.add_argument("--radius", type=int, default=4)
    ap.add_argument("--eps", type=float, default=1e-4)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--quality_image", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("guided_bench needs a ROCm device")
    from upr import calib
    res = {"metric": "guided-filter restore (upr.guided.fit / apply), device-event time per call",
           "hbm_TBps_for_floors": HBM_TBPS,
           "hbm_copy_TBps_this_run": calib.measure(torch.device("cuda"), warm_s=0.5)["hbm_copy_TBps"],
           "workloads": [measure(n, size, args.max_size, args.reps, args.radius, args.eps)
                         for n, size in ((32, 1024), (8, 2048))]}
    if args.quality or args.quality_image:
        res["quality"] = quality(args.quality_image, args.max_size, args.radius, args.eps)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
