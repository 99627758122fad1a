#!/usr/bin/env python3
"""SURVEY §8f ranks 2-3 on the device, timed with HIP events on the launching
stream (torch's current stream), one JSON line each:

  content_aware  ContentAwareEnhancer.apply_content_aware_enhancement's device
                 part (enhancers/content_aware.py:19-122) over a resident
                 B x 3 x S x S fp32 batch: upr_content_aware (gray -> |Laplacian|
                 -> 15x15 Gaussian (fp64, like the reference's CV_64F) ->
                 min-max -> attention -> clamp(enh * (1 + 0.2 att))).
                 Algorithmic bytes: x read once, enh read once, out written
                 once = 36 B/px; the fp64 maps between the passes are not
                 algorithmic (the pass bytes are reported beside it).
  letterbox      utils/letterbox.py:9-102 (INTER_LINEAR resize + grey-114 pad +
                 /255) of decoded u8 HWC frames, one upr_letterbox launch per
                 frame; algorithmic bytes = u8 in + fp32 [3,H',W'] out.

  python tools/enh_extra_bench.py [--batch 32] [--size 512] [--frames 32]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "retinex-image-enhancement_amd"))

import torch  # noqa: E402

PEAK_HBM_GBS = 8000.0


def timed(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    from upr import runtime
    from utils.letterbox import letterbox_u8_image
    dev = torch.device("cuda", 0)
    B, S = args.batch, args.size
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.rand(B, 3, S, S, device=dev, generator=g) * 0.4
    enh = torch.rand(B, 3, S, S, device=dev, generator=g)
    ms = timed(lambda: runtime.content_aware(x, enh), args.iters)
    px = B * S * S
    alg = 36.0 * px
    # bytes the passes move (partials negligible); the three-kernel form: lap (x 12 in, 8 out), gauss rows
    # (8 / 8), gauss cols (8 / 8), att (x 12 + lap 8 in, att 4 out), apply (att 4 + enh 12 in, 12 out)
    fused = (S * S) % 4 == 0
    # fused: saliency (x 12 in, fp64 map 8 out), att (map 8 + x 12 in, att 4 out), apply (att 4 + enh 12 in, 12 out)
    passes = (12 + 8) + (8 + 12 + 4) + (4 + 12 + 12) if fused else \
        (12 + 8) + (8 + 8) + (8 + 8) + (12 + 8 + 4) + (4 + 12 + 12)
    print(json.dumps({"what": "content_aware", "batch": B, "size": S, "ms_per_call": ms, "images_per_s": B / ms * 1e3,
                      "alg_bytes": alg, "achieved_GBs": alg / ms / 1e6, "frac_hbm": alg / ms / 1e6 / PEAK_HBM_GBS,
                      "pass_bytes_per_px": passes, "pass_GBs": passes * px / ms / 1e6,
                      "kernels": ("ca_sal_fused, ca_att4, ca_apply4 (each reducing its producer's min / max partials)"
                                  if fused else "ca_lap, ca_gauss_rows, ca_gauss_cols, reduce_minmax<double>, ca_att, "
                                                "reduce_minmax<float>, ca_apply")}))
    # letterbox: 1920 x 1080 u8 frames -> 640 (the reference default new_shape), auto padding
    import numpy as np
    frames = [np.random.default_rng(k).integers(0, 256, (1080, 1920, 3), dtype=np.uint8) for k in range(4)]
    dframes = [torch.from_numpy(f).to(dev) for f in frames]
    from utils.letterbox import _run
    outs = []

    def lb():
        outs.clear()
        for k in range(args.frames):
            t = dframes[k % len(dframes)]
            outs.append(_run(t, 0, 1080, 1920, 640, (114, 114, 114), True, False, True, 0)[0])
    ms = timed(lb, max(args.iters // 4, 3))
    o = outs[0]
    lb_alg = args.frames * (1080 * 1920 * 3 + o.numel() * 4)
    print(json.dumps({"what": "letterbox", "frames": args.frames, "src": "1080x1920 u8 HWC", "dst": list(o.shape),
                      "ms_per_frame": ms / args.frames, "frames_per_s": args.frames / ms * 1e3,
                      "alg_bytes_per_frame": lb_alg / args.frames, "achieved_GBs": lb_alg / ms / 1e6,
                      "frac_hbm": lb_alg / ms / 1e6 / PEAK_HBM_GBS,
                      "note": "one launch per frame (the harness letterboxes each decoded file); the OpenCV "
                              "tap tables are built once per (size, device) and kept on the device "
                              "(utils/letterbox.py _device_taps)"}))
    _ = letterbox_u8_image  # the harness path (decoded bytes in) uses the same kernel


if __name__ == "__main__":
    main()
