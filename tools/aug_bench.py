#!/usr/bin/env python3
"""Training data path on one GPU: the augment call against its byte floor, and
the loader against the training step.

(a) upr_augment, all six stages on (generated noise), 8 x 3 x 512^2 and
    8 x 3 x 640^2, k = 0 (row kernel) and k = 1 (LDS transpose): HIP events,
    warm-up, median of --reps calls.  Beside each: the call's algorithmic bytes
    (12 B/px read + 12 written + 12 read by the statistics pass) at the copy
    rate upr_calib_run(UPR_CALIB_HBM_COPY) reaches in this process.
(b) batches per second of get_train_dataloader over a directory of PNGs written
    into a temporary folder, per decode-thread count, with the per-image cost
    of each stage (decode, upload, letterbox) and the per-batch augment call;
    beside it the training step's img/s from `bench.py --train --amp`, run as a
    child process before this one opens the GPU.

Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "retinex-image-enhancement_amd"), REPO]


def step_rate(steps, warmup):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--train", "--amp", "--steps", str(steps),
           "--warmup", str(warmup), "--cpu-seconds", "0", "--no-traffic", "--no-profile"]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py exited with {r.returncode}: {r.stderr[-2000:]}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    return {"img_per_s": d["value"], "ms_per_step": d["ms_per_step"], "metric": d["metric"], "command": " ".join(cmd[1:])}


def event_ms(fn, warm, reps):
    import torch
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def copy_rate(dev):
    """read + write bytes per second of the best streaming copy form (upr.calib's HBM part)."""
    import ctypes
    import torch
    from upr import _lib as L
    from upr import calib
    lib, n = L.lib(), 1 << 30
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    a = torch.empty(n, dtype=torch.uint8, device=dev).random_(0, 255)
    b = torch.empty_like(a)
    best = 0.0
    for mode in (0, 1, 2):
        for blocks in (1024, 2048, 4096):
            calib._run(lib, L.UPR_CALIB_HBM_COPY, blocks, mode, a, b, n, 5, stream)
            ms = calib._run(lib, L.UPR_CALIB_HBM_COPY, blocks, mode, a, b, n, 50, stream)
            best = max(best, 2.0 * n / (ms * 1e-3))
    return best


def entry_call(x, y, rec, dev, seed=1):
    """-> a closure making one upr_augment call with the records already on the device."""
    import ctypes
    import torch
    from upr import _lib as L
    lib = L.lib()
    B, _, H, W = x.shape
    ws = torch.empty(lib.upr_augment_workspace(B, H, W), dtype=torch.uint8, device=dev)
    rec_dev = rec.to(dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    args = (x.data_ptr(), y.data_ptr(), B, H, W, rec_dev.data_ptr(), rec.data_ptr(), seed, None, ws.data_ptr(),
            ws.numel(), stream)

    def call(keep=(ws, rec_dev, rec)):
        rc = lib.upr_augment(*args)
        if rc:
            raise RuntimeError(f"upr_augment: {rc}")
    return call


def kernel_part(dev, reps):
    import torch
    from upr import augment as A
    rate = copy_rate(dev)
    rows = []
    for size in (512, 640):
        x = (torch.rand(8, 3, size, size, device=dev) * 0.5).contiguous()
        y = torch.empty_like(x)
        for k in (0, 1):
            p = {"hflip": True, "vflip": False, "k": k, "gamma": 1.3, "contrast": 1.1, "brightness": 0.03,
                 "noise_level": 0.02, "saturation": 1.1, "shift": -0.01}
            ids = list(range(8))
            rec = A.pack([p] * 8, ids)
            med = {}
            ms = event_ms(entry_call(x, y, rec, dev), 10, reps)
            med["all"] = statistics.median(ms)
            # where the time goes: the same call without the statistics pass, without the generator, bare
            variants = {"no_contrast": dict(p, contrast=None), "no_noise": dict(p, noise_level=None),
                        "geometry_only": dict(p, gamma=None, contrast=None, brightness=None, noise_level=None,
                                              saturation=None, shift=None)}
            for name, q in variants.items():
                med[name] = statistics.median(event_ms(entry_call(x, y, A.pack([q] * 8, ids), dev), 10, reps))
            with_upload = statistics.median(event_ms(lambda: A.augment(x, rec, seed=1, out=y), 10, reps))
            px = 8.0 * size * size
            floor_ms = 36.0 * px / rate * 1e3
            rows.append({"shape": [8, 3, size, size], "k": k, "stages": "all six, generated noise", "reps": reps,
                         "call_ms_median": med["all"], "call_ms_min": min(ms), "call_ms_max": max(ms),
                         "alg_bytes": 36.0 * px, "floor_ms_at_copy_rate": floor_ms,
                         "time_over_floor": med["all"] / floor_ms,
                         "python_call_with_record_upload_ms_median": with_upload,
                         "no_contrast_ms_median": med["no_contrast"], "no_noise_ms_median": med["no_noise"],
                         "geometry_only_ms_median": med["geometry_only"],
                         "floor_ms_24B_per_px": 24.0 * px / rate * 1e3})
    return {"hbm_copy_TBps": rate / 1e12, "calls": rows,
            "note": "call = one upr_augment entry (statistics pass + finish + apply pass; records resident), HIP "
                    "events on the stream; floor = 36 B/px at the measured copy rate (24 B/px without the "
                    "statistics pass: no_contrast, geometry_only); python_call adds upr.augment.augment's "
                    "record upload from pinned memory"}


def write_pngs(folder, n, size):
    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(0)
    yy, xx = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    for i in range(n):
        base = np.stack([(xx * (i + 1) + yy) % 256, (yy * 2 + i * 7) % 256, (xx + yy * (i % 5)) % 256], axis=2)
        img = (base * 0.35 + rng.integers(0, 24, base.shape)).astype(np.uint8)  # dark, smooth + sensor-like noise
        Image.fromarray(img).save(os.path.join(folder, f"low{i:03d}.png"))


def loader_part(dev, size, batch, n_images, workers):
    import numpy as np
    import torch
    from datasets.dataset import decode_u8, get_train_dataloader
    from utils.letterbox import letterbox_u8_image
    out = {"image_size": size, "batch_size": batch, "images": n_images, "format": "PNG, written by this tool"}
    with tempfile.TemporaryDirectory() as folder:
        write_pngs(folder, n_images, size)
        files = sorted(os.path.join(folder, f) for f in os.listdir(folder))
        t0 = time.perf_counter()
        imgs = [decode_u8(f) for f in files[:16]]
        out["decode_ms_per_image_one_thread"] = (time.perf_counter() - t0) / 16 * 1e3
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for im in imgs:
            torch.from_numpy(np.ascontiguousarray(im)).to(dev)
        torch.cuda.synchronize()
        out["upload_ms_per_image"] = (time.perf_counter() - t0) / 16 * 1e3
        dst = torch.empty(3, size, size, device=dev)
        lb = event_ms(lambda: [letterbox_u8_image(im, size, auto=True, scaleup=True, device=dev, out=dst)
                               for im in imgs], 2, 5)
        out["upload_plus_letterbox_ms_per_image"] = statistics.median(lb) / 16
        out["loader"] = []
        for nw in workers:
            ld = get_train_dataloader(folder, batch_size=batch, image_size=size, num_workers=nw,
                                      advanced_augment=True, device=dev, seed=0)
            rates = []
            for epoch in range(4):  # the first epoch warms the file cache, the kernels and the allocator
                ld.set_epoch(epoch)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                nb = 0
                for b in ld:
                    nb += 1
                torch.cuda.synchronize()
                if epoch:
                    rates.append(nb / (time.perf_counter() - t0))
            r = statistics.median(rates)
            out["loader"].append({"num_workers": nw, "batches_per_s": r, "img_per_s": r * batch,
                                  "epochs_timed": len(rates), "min": min(rates), "max": max(rates)})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=21, help="timed augment calls per case (median reported, >= 5)")
    ap.add_argument("--size", type=int, default=512, help="loader image size (the step benchmark's)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--workers", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-step", action="store_true", help="skip the bench.py --train --amp child run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    res = {"tool": "tools/aug_bench.py"}
    res["train_step"] = None
    if not args.no_step:  # before this process opens the GPU
        try:
            res["train_step"] = step_rate(args.steps, args.warmup)
        except Exception as e:  # the rest is still worth having; the record says what is missing
            res["train_step_error"] = str(e)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("aug_bench needs a ROCm device: nothing is measured without one")
    dev = torch.device("cuda", 0)
    res["device"] = torch.cuda.get_device_name(dev)
    res["augment"] = kernel_part(dev, args.reps)
    res["data_path"] = loader_part(dev, args.size, args.batch, args.images, args.workers)
    if res["train_step"]:
        best = max(r["img_per_s"] for r in res["data_path"]["loader"])
        res["slower_side"] = "loader" if best < res["train_step"]["img_per_s"] else "step"
        res["loader_over_step"] = best / res["train_step"]["img_per_s"]
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
