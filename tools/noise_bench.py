#!/usr/bin/env python3
"""Blind denoising (upr.denoise.estimate_sigma / nlm with per-image tables / nlm_auto): op times,
and what --denoise_strength auto costs the directory harness.

  python tools/noise_bench.py [--rounds 10] [--harness_rounds 3] [--parent_lib FILE]
                              [--out profiles/denoise_auto_v1.json]

Estimator: 8 x and 32 x 512^2 images, the harness bench's noisy images (tools/denoise_bench.py
noisy_images) and a constant image (every sample in bin 0: the contention case), against the
floor of 3 B read per pixel over 6.29 TB/s, the copy rate measured for this part.
Filter: upr_denoise_nlm_u8 (the table a kernel argument) against upr_denoise_nlm_u8_luts (a
table per image in device memory, all rows that same table) at (search, patch) = (5, 2) and
(3, 1), 32 x 512^2; and nlm_auto, the three launches together.
--parent_lib: another build of libupr.so (the parent commit's); its upr_denoise_nlm_u8 is
called with the same arguments, alternating with this tree's.
One call between device events per configuration and round, the configurations alternating
inside a round; medians over --rounds after a warm-up of every configuration.

Harness: tools/harness_bench.py run() on one directory of 32 noisy 512^2 PNGs at batch 32,
denoise off / nlm at strength 1.0 / nlm at strength auto alternating, --harness_rounds times
each after one uncounted round: images/s as median and range, host and device PNG encoder.
"""
import argparse
import ctypes
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
from denoise_bench import HBM_TBPS, noisy_images  # noqa: E402


def _timed(configs, rounds):
    for c in configs:  # warm-up: code objects, allocator
        for _ in range(3):
            c["call"]()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for c in configs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            c["call"]()
            e1.record()
            e1.synchronize()
            c["ms"].append(e0.elapsed_time(e1))
    out = []
    for c in configs:
        row = {k: v for k, v in c.items() if k not in ("call", "ms")}
        row |= {"ms_median": statistics.median(c["ms"]), "ms_min": min(c["ms"]), "ms_max": max(c["ms"]),
                "rounds": rounds}
        out.append(row)
    return out


def op_times(rounds, parent_lib):
    from upr import _lib as L, denoise
    from upr.runtime import _ptr, _stream
    configs = []
    for n in (8, 32):
        for name, imgs in (("noisy", noisy_images(n, 512)), ("constant", np.full((n, 512, 512, 3), 90, np.uint8))):
            x = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
            configs.append(dict(op="estimate_sigma", images=n, size=512, data=name, ms=[],
                                call=lambda x=x: denoise.estimate_sigma(x)))
    x = torch.from_numpy(noisy_images(32, 512)).cuda()
    m = x.float().mean(3, keepdim=True).round().to(torch.uint8).expand(-1, -1, -1, 3).contiguous()
    out = torch.empty_like(x)
    ones = torch.ones(32, dtype=torch.float64, device="cuda")
    parent = None
    if parent_lib:
        parent = ctypes.CDLL(parent_lib)
        parent.upr_denoise_nlm_u8.restype = ctypes.c_int
        parent.upr_denoise_nlm_u8.argtypes = L.lib().upr_denoise_nlm_u8.argtypes
    for search, patch in ((5, 2), (3, 1)):
        table = denoise.lut(1.0, 16, patch)
        tables = denoise.lut_device(ones, 1.0, 16, patch)
        common = dict(images=32, size=512, data="noisy", search=search, patch=patch)

        def fixed(lib, search=search, patch=patch, table=table):
            rc = lib.upr_denoise_nlm_u8(_ptr(x), _ptr(m), 3, 32, 512, 512, 0, 0, 512, 512, search, patch, table,
                                        _ptr(out), _stream(x.device))
            assert rc == 0, rc

        def rows(search=search, patch=patch, tables=tables):
            rc = L.lib().upr_denoise_nlm_u8_luts(_ptr(x), _ptr(m), 3, 32, 512, 512, 0, 0, 512, 512, search, patch,
                                                 _ptr(tables), _ptr(out), _stream(x.device))
            assert rc == 0, rc

        configs.append(dict(common, op="nlm_u8 (argument table)", ms=[], call=lambda f=fixed: f(L.lib())))
        if parent is not None:
            configs.append(dict(common, op="nlm_u8 (argument table), parent build", ms=[],
                                call=lambda f=fixed: f(parent)))
        configs.append(dict(common, op="nlm_u8_luts (a table per image)", ms=[], call=rows))
        configs.append(dict(common, op="nlm_auto (estimate + tables + filter)", ms=[],
                            call=lambda s=search, p=patch: denoise.nlm_auto(x, x, m, None, 1.0, 16, s, p, out=out)))
    res = _timed(configs, rounds)
    for r in res:
        if r["op"] == "estimate_sigma":
            floor = r["images"] * r["size"] ** 2 * 3 / (HBM_TBPS * 1e12) * 1e3
            r["hbm_floor_ms"], r["ratio_to_hbm_floor"] = floor, r["ms_median"] / floor
    return res


def harness(rounds):
    res = []
    modes = {"off": dict(denoise="off"), "nlm_fixed": dict(denoise="nlm"),
             "nlm_auto": dict(denoise="nlm", denoise_strength="auto")}
    with tempfile.TemporaryDirectory(dir="/tmp") as d:
        src = os.path.join(d, "in")
        harness_bench.write_inputs(src, 32, 512)
        for encoder in ("host", "device"):
            rates, written, stages = {k: [] for k in modes}, {}, {k: [] for k in modes}
            for rnd in range(rounds + 1):  # round 0 warms every mode and is not counted
                for mode, kw in modes.items():
                    r = harness_bench.run(src, os.path.join(d, f"out_{encoder}_{mode}{rnd}"), 32, 512,
                                          png_encoder=encoder, batch_size=32, warm=False, **kw)
                    assert r["files_written"] == 96, r
                    if rnd:
                        rates[mode].append(r["value"])
                        stages[mode].append(r["stage_seconds"])
                        written[mode] = r["output_bytes"]  # (the modes write different pixels: different files)
            row = {"png_encoder": encoder, "batch_size": 32, "n": 32, "size": 512, "rounds": rounds,
                   "unit": "images/s"}
            for mode, v in rates.items():
                row[mode] = {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v,
                             "output_bytes": written[mode], "stage_seconds": stages[mode]}
            res.append(row)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--harness_rounds", type=int, default=3)
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("noise_bench needs a ROCm device")
    res = {"metric": "blind denoising: device-event time per call of the estimator, the filter with the table as an "
                     "argument / per image / measured, and the directory harness with denoise off / fixed / auto",
           "hbm_TBps_for_floors": HBM_TBPS, "parent_lib": bool(args.parent_lib),
           "op": op_times(args.rounds, args.parent_lib)}
    if args.harness_rounds > 0:
        res["harness"] = harness(args.harness_rounds)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
