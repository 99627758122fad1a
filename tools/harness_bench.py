#!/usr/bin/env python3
"""End-to-end `main.py --mode enhance` directory throughput (decode -> device
letterbox -> model + CLAHE-in-Lab enhancer -> device u8 -> PNG encode):
enhance_batch_images over N synthetic low-light PNGs, images/s including IO.

  python tools/harness_bench.py --n 32 --size 512 [--precision fp16] [--png_encoder device|device_lz]
                                [--batch_size 32 [--decode_threads 4]] [--mixed]
                                [--image_format jpg [--jpeg_quality 95] [--jpeg_subsampling 420] [--jpeg_optimize]
                                 [--jpeg_gray_maps] [--jpeg_modes_compare [--rounds 3] [--out FILE]]]
                                [--max_size 512 [--output_size original]] [--restore_compare [--rounds 3]]
                                [--denoise nlm]

--batch_size > 1 runs the batched path and adds its per-stage wall-time sums
(`stage_seconds`) to the JSON; --mixed writes images of --size and of half of it,
interleaved, so the batches are formed from two shape buckets.  --image_format jpg
writes the three output files per image as JPEGs (PIL with the host encoder, upr.jpeg
with a device encoder) and adds the bytes written to the JSON.  --max_size M letterboxes to M;
--output_size original writes the files at the sources' size (the guided-filter restore).
--jpeg_modes_compare times --image_format jpg alone against the same with --jpeg_subsampling 420
--jpeg_optimize --jpeg_gray_maps on one directory, alternating, --rounds times each: bytes written
and images/s as median and range.
--restore_compare times the two routes to source-sized files on the same directory, alternating,
--rounds times each: `--max_size M --output_size original` against no --max_size (the forward at
the sources' own size); images/s as median and range of the rounds.
--denoise nlm passes denoise="nlm" on (upr.denoise at its defaults; tools/denoise_bench.py
alternates it with off).
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "retinex-image-enhancement_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402


def write_inputs(src, n, size, mixed=False):
    os.makedirs(src)
    rng = np.random.default_rng(0)
    for k in range(n):
        s = size // 2 if mixed and k % 2 else size
        a = (rng.integers(0, 256, (s, s, 3)) * 0.35).astype(np.uint8)
        Image.fromarray(a).save(os.path.join(src, f"img{k:03d}.png"))


def run(src, out, n, size, precision="fp32", png_encoder="host", batch_size=1, decode_threads=4, mixed=False,
        warm=True, image_format="png", jpeg_quality=95, max_size=None, output_size="letterbox",
        jpeg_subsampling="444", jpeg_optimize=False, jpeg_gray_maps=False, denoise="off", denoise_strength=None):
    """One timed enhance_batch_images over the files of `src` -> the result dict."""
    from enhancers.simple_enhance import enhance_batch_images
    kw = {"png_encoder": png_encoder} if png_encoder != "host" else {}
    if image_format != "png":
        kw.update(image_format=image_format, jpeg_quality=jpeg_quality)
        if (jpeg_subsampling, jpeg_optimize, jpeg_gray_maps) != ("444", False, False):
            kw.update(jpeg_subsampling=jpeg_subsampling, jpeg_optimize=jpeg_optimize, jpeg_gray_maps=jpeg_gray_maps)
    if max_size is not None:
        kw["max_size"] = max_size
    if output_size != "letterbox":
        kw["output_size"] = output_size
    if denoise != "off":
        kw["denoise"] = denoise
        if denoise_strength is not None:  # a number or "auto" (tools/noise_bench.py)
            kw["denoise_strength"] = denoise_strength
    timings = None
    if batch_size != 1:
        timings = {}
        kw.update(batch_size=batch_size, decode_threads=decode_threads)
    with contextlib.redirect_stdout(io.StringIO()):
        if warm:  # packing, allocator pools, pinned buffers
            enhance_batch_images(src, out + "_warm", "cuda", seed=0, precision=precision, **kw)
        if timings is not None:
            kw["timings"] = timings
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enhance_batch_images(src, out, "cuda", seed=0, precision=precision, **kw)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
    res = {"metric": "enhance harness images/s (decode + letterbox + UP_Retinex preact+ASPP + "
                     "CLAHE-in-Lab + 3 PNG writes per image)", "value": n / el, "unit": "images/s",
           "n": n, "size": size, "precision": precision, "png_encoder": png_encoder,
           "batch_size": batch_size, "mixed": bool(mixed), "seconds": el, "files_written": len(os.listdir(out)),
           "image_format": image_format, "max_size": max_size, "output_size": output_size,
           "denoise": denoise, "denoise_strength": denoise_strength,
           "output_bytes": sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out))}
    if image_format == "jpg":
        res["jpeg_quality"] = jpeg_quality
        res.update(jpeg_subsampling=jpeg_subsampling, jpeg_optimize=jpeg_optimize, jpeg_gray_maps=jpeg_gray_maps)
    if timings is not None:
        res["decode_threads"] = decode_threads
        res["stage_seconds"] = {k: round(v, 6) for k, v in sorted(timings.items())}
    return res


def restore_compare(src, out, args):
    """Alternating runs of the restore route and the full-size route on one directory."""
    import statistics
    routes = {"restore": dict(max_size=args.max_size or 512, output_size="original"), "full_size": {}}
    common = dict(precision=args.precision, png_encoder=args.png_encoder, batch_size=args.batch_size,
                  decode_threads=args.decode_threads, image_format=args.image_format, jpeg_quality=args.jpeg_quality)
    rates = {k: [] for k in routes}
    for rnd in range(args.rounds + 1):  # round 0 warms both routes and is not counted
        for name, kw in routes.items():
            r = run(src, f"{out}_{name}{rnd}", args.n, args.size, warm=False, **common, **kw)
            assert r["files_written"] == 3 * args.n, r
            if rnd:
                rates[name].append(r["value"])
    res = {"metric": "enhance harness images/s to source-sized files: --max_size M --output_size original against "
                     "the forward at the sources' own size, alternating runs", "unit": "images/s", "n": args.n,
           "size": args.size, "rounds": args.rounds, **common, "restore_max_size": routes["restore"]["max_size"]}
    for name, v in rates.items():
        res[name] = {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}
    res["restore_over_full_size"] = res["restore"]["median"] / res["full_size"]["median"]
    return res


def jpeg_modes_compare(src, out, args):
    """Alternating runs of the default JPEG files and of 4:2:0 + optimised tables + gray maps."""
    import statistics
    routes = {"jpg_444_standard": {}, "jpg_420_optimize_gray_maps": dict(jpeg_subsampling="420", jpeg_optimize=True,
                                                                         jpeg_gray_maps=True)}
    common = dict(precision=args.precision, png_encoder=args.png_encoder, batch_size=args.batch_size,
                  decode_threads=args.decode_threads, image_format="jpg", jpeg_quality=args.jpeg_quality)
    runs = {k: [] for k in routes}
    for rnd in range(args.rounds + 1):  # round 0 warms both routes and is not counted
        for name, kw in routes.items():
            r = run(src, f"{out}_{name}{rnd}", args.n, args.size, warm=False, **common, **kw)
            assert r["files_written"] == 3 * args.n, r
            if rnd:
                runs[name].append(r)
    res = {"metric": "enhance harness images/s and bytes written, --image_format jpg alone against the same with "
                     "--jpeg_subsampling 420 --jpeg_optimize --jpeg_gray_maps, alternating runs", "unit": "images/s",
           "n": args.n, "size": args.size, "rounds": args.rounds, **common}
    for name, rs in runs.items():
        v = [r["value"] for r in rs]
        res[name] = {"images_per_s_median": statistics.median(v), "images_per_s_min": min(v),
                     "images_per_s_max": max(v), "images_per_s_runs": v, "output_bytes": rs[0]["output_bytes"],
                     "stage_seconds_runs": [r.get("stage_seconds") for r in rs]}
    res["bytes_ratio"] = res["jpg_420_optimize_gray_maps"]["output_bytes"] / res["jpg_444_standard"]["output_bytes"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--precision", choices=["fp32", "fp16"], default="fp32")
    ap.add_argument("--png_encoder", choices=["host", "device", "device_lz"], default="host")
    ap.add_argument("--batch_size", type=int, default=1)
    ap.add_argument("--decode_threads", type=int, default=4)
    ap.add_argument("--mixed", action="store_true")
    ap.add_argument("--image_format", choices=["png", "jpg"], default="png")
    ap.add_argument("--jpeg_quality", type=int, default=95)
    ap.add_argument("--jpeg_subsampling", choices=["444", "420"], default="444")
    ap.add_argument("--jpeg_optimize", action="store_true")
    ap.add_argument("--jpeg_gray_maps", action="store_true")
    ap.add_argument("--jpeg_modes_compare", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--max_size", type=int, default=None)
    ap.add_argument("--output_size", choices=["letterbox", "original"], default="letterbox")
    ap.add_argument("--restore_compare", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--denoise", choices=["off", "nlm"], default="off")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory(dir="/tmp") as d:
        src, out = os.path.join(d, "in"), os.path.join(d, "out")
        write_inputs(src, args.n, args.size, args.mixed)
        if args.restore_compare:
            res = restore_compare(src, out, args)
        elif args.jpeg_modes_compare:
            res = jpeg_modes_compare(src, out, args)
        else:
            res = run(src, out, args.n, args.size, args.precision, args.png_encoder, args.batch_size,
                      args.decode_threads, args.mixed, image_format=args.image_format,
                      jpeg_quality=args.jpeg_quality, max_size=args.max_size, output_size=args.output_size,
                      jpeg_subsampling=args.jpeg_subsampling, jpeg_optimize=args.jpeg_optimize,
                      jpeg_gray_maps=args.jpeg_gray_maps, denoise=args.denoise)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
