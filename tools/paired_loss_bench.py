#!/usr/bin/env python3
"""Paired loss terms (upr_t_loss_paired, csrc/train_paired.hip): the op against its HBM floor, and what
the paired terms add to an AMP training step.

  python tools/paired_loss_bench.py [--reps 20] [--steps 10] [--out profiles/paired_loss_v1.json]

Op: enh / target uniform noise at 8x3x512^2 and 32x3x512^2, gradients on (g_enh accumulated into).
Time is HIP events around a burst of --reps calls on the launching stream (both launches of a call and
their host cost included), per call.  The floor is 16 B per element -- read enh and target,
read-modify-write g_enh -- over 6.29 TB/s, the copy rate measured for this part (the other tools quote
the same rate).

Step: trainers.train.train_step under AMP (GradScaler, fp16 autocast) at batch 8, 512^2, on one fixed
batch, the plain model (no preact, no ASPP) and TotalLoss's defaults, with TotalLoss(weight_rec=1,
weight_ssim=1) and a target against the same criterion without one; wall time of --steps steps after a
synchronisation, per step.

Every configuration is measured in three rounds that alternate between the configurations, in one
process; the record holds the three values, their median and their range.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "retinex-image-enhancement_amd"))

import torch  # noqa: E402

HBM_TBPS = 6.29
ROUNDS = 3


def summary(values):
    return {"rounds": values, "median": statistics.median(values), "min": min(values), "max": max(values)}


def op_round(x, y, g, reps):
    from upr.loss_engine import paired_terms
    out2 = torch.empty(2, dtype=torch.float32, device=x.device)
    for _ in range(3):
        paired_terms(x, y, out2=out2, g_enh=g)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        paired_terms(x, y, out2=out2, g_enh=g)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def measure_op(reps):
    cases = []
    for B in (8, 32):
        gen = torch.Generator(device="cuda").manual_seed(B)
        x = torch.rand(B, 3, 512, 512, device="cuda", generator=gen)
        y = torch.rand(B, 3, 512, 512, device="cuda", generator=gen)
        cases.append((B, x, y, torch.zeros_like(x)))
    ms = {B: [] for B, *_ in cases}
    for _ in range(ROUNDS):
        for B, x, y, g in cases:
            ms[B].append(op_round(x, y, g, reps))
    out = []
    for B, x, *_ in cases:
        floor = x.numel() * 16 / (HBM_TBPS * 1e12) * 1e3
        s = summary(ms[B])
        out.append({"shape": [B, 3, 512, 512], "gradients": True, "calls_per_round": reps, "ms_per_call": s,
                    "hbm_floor_ms": floor, "share_of_hbm_floor": floor / s["median"],
                    "achieved_GBs": x.numel() * 16 / (s["median"] * 1e-3) / 1e9})
    return out


def step_round(model, crit, opt, scaler, low, target, steps):
    from trainers.train import train_step
    for _ in range(2):
        train_step(model, low, crit, opt, scaler=scaler, use_amp=True, target=target)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        train_step(model, low, crit, opt, scaler=scaler, use_amp=True, target=target)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def measure_step(steps):
    from losses.loss import TotalLoss
    from models.model import MultiScaleUP_Retinex
    from trainers.train import GradScaler, make_optimizer
    torch.manual_seed(0)
    model = MultiScaleUP_Retinex(use_preact=False, use_aspp=False).to("cuda").train()
    opt = make_optimizer(model)
    scaler = GradScaler()
    gen = torch.Generator(device="cuda").manual_seed(1)
    target = torch.rand(8, 3, 512, 512, device="cuda", generator=gen)
    low = target * 0.3
    crits = {"unpaired": (TotalLoss().to("cuda"), None),
             "paired": (TotalLoss(weight_rec=1.0, weight_ssim=1.0).to("cuda"), target)}
    ms = {k: [] for k in crits}
    for _ in range(ROUNDS):
        for k, (crit, t) in crits.items():
            ms[k].append(step_round(model, crit, opt, scaler, low, t, steps))
    res = {k: summary(v) for k, v in ms.items()}
    return {"batch": 8, "size": 512, "amp": True, "model": "MultiScaleUP_Retinex (no preact, no ASPP)",
            "steps_per_round": steps, "ms_per_step": res,
            "paired_minus_unpaired_ms": res["paired"]["median"] - res["unpaired"]["median"],
            "paired_over_unpaired": res["paired"]["median"] / res["unpaired"]["median"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip_step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rec = {"what": "upr_t_loss_paired", "device": torch.cuda.get_device_name(0), "hbm_TBps": HBM_TBPS,
           "rounds": ROUNDS,
           "timing": "op: HIP events around a burst of calls; step: wall time of a run of steps between "
                     "synchronisations; configurations alternate round by round in one process",
           "kernel": "16 x 32 tile per block, 256 threads, 77184 B LDS (2 blocks per CU), window sums and both "
                     "box passes in fp64",
           "op": measure_op(args.reps)}
    if not args.skip_step:
        rec["train_step"] = measure_step(args.steps)
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
