#!/usr/bin/env python3
"""UP-Retinex hot-path benchmark (BASELINE.json metric: images/s at 512x512 bs=32).

One step = one MultiScaleUP_Retinex forward over one resident batch of 32
synthetic 512x512 images per GPU.  The headline (`value`) is configs[1]
(random-init plain model, fp32); `--precision fp16 --variant preact_aspp`
makes configs[2] the headline instead.

A plain run (`--gpus 1 --steps N --warmup W`) does only what the headline
needs: it builds the seeded model and inputs, warms up, times the N steps,
writes the last step's outputs when `--dump-outputs DIR` is given, and prints
the line (with the roofline object from the per-launch events of the last
timed step).  Everything else is behind `--full`: the PMC traffic passes,
parity against the CPU oracle, the CPU baselines, and (unless --no-nested)
three nested objects on the same JSON line, each with its own roofline, parity
and CPU baseline:
  fp16_preact_aspp  configs[2]: bs 32 512^2 fp16 preact+ASPP forward
  enhance           the enhancers main.py --mode enhance runs after the model (CLAHE-in-Lab,
                    multi-scale factor + clamp) over a resident bs 32 512^2 batch (`--enhance`
                    makes it the headline)
  train_amp         configs[4]: bs 8 512^2 AMP training step (rank 0 of an N=1
                    run only; `--train` makes it the headline)

Multi-GPU: one process per GPU.  `--gpus N` (N > 1) run directly makes this
process a pure launcher (it never touches the GPU): it starts
`torch.distributed.run` with N ranks on 127.0.0.1 and exits with its code; run
under torch.distributed.run (WORLD_SIZE set) it is one rank.  Each rank
processes its own 32-image shard with no data-path collective (weak scaling);
`--collect all|rank0` adds the final collect of SURVEY §8e inside the timed
region (RCCL all_gather_into_tensor to every rank, or a gather to rank 0 only,
of the fp16 enhanced images).  Barrier + synchronize bracket the timed region
and rank 0 reports the max over ranks.  `--dry-run` replaces the GPU work by a
small CPU step over gloo and emits the same keys (tests the launcher / rank /
report plumbing on a machine without a GPU).

Extra objects on the JSON line (traffic, parity and cpu_baseline with --full only):
  roofline      the conv kernel family (CONV_KERNELS below, ~97% of device time), timed live with HIP events around every
                launch of the last timed step on the model's stream
                (upr_model_profile); traffic from rocprofv3 FETCH_SIZE/WRITE_SIZE
                child passes run before this process touches the GPU (N=1 only:
                the numbers are per rank, and the passes need the whole GPU);
                --ceilings adds the fractions against measured MFMA / HBM rates
  parity        images 0 and B-1 of rank 0's last timed batch vs the CPU oracle, at any world size
  cpu_baseline  the CPU oracle (oracle/net.py, torch-CPU fp32) on the host cores this process may use,
                rank 0 of an N=1 run only: 1 warm-up image, then the median of 3 timed repetitions of the sample
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(REPO, "retinex-image-enhancement_amd")
for _p in (PKG, REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

PEAK_TFLOPS = {"fp32": 157.3, "fp16": 2516.6}   # MI355X dense MFMA (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0
REF_GFLOP_PER_IMG = {"plain": 105.6, "preact_aspp": 123.4}
TRAIN_GFLOP_PER_IMG = 668.0  # model fwd+bwd + VGG19 fwd x2 + dgrad, 512x512
CPU_REPS = 3


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32, help="images per GPU")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--precision", choices=["fp32", "fp16"], default="fp32")
    ap.add_argument("--variant", choices=["plain", "preact_aspp"], default="plain")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="0 = skip the CPU baselines")
    ap.add_argument("--no-profile", action="store_true", help="skip per-launch HIP events")
    ap.add_argument("--breakdown", action="store_true", help="print per-layer stats to stderr")
    ap.add_argument("--no-traffic", action="store_true", help="skip the rocprofv3 PMC traffic passes")
    ap.add_argument("--no-nested", action="store_true",
                    help="only the headline config (no fp16_preact_aspp / train_amp objects)")
    ap.add_argument("--ceilings", action="store_true",
                    help="after the timed steps, measure the chip's reachable fp16 MFMA and HBM-copy rates "
                         "(upr/calib.py, ~5 s) and report the roofline fractions against them as well")
    ap.add_argument("--train", action="store_true",
                    help="configs[4] as the headline: one training step (fwd + TotalLoss + bwd + clip + Adam) per "
                         "step, bs=8 512x512 plain model (batch/size overridable)")
    ap.add_argument("--collect", nargs="?", const="all", default="none", choices=["none", "all", "rank0"],
                    help="time the final collect too: fp16 enhanced images to every rank (all) or to rank 0")
    ap.add_argument("--dry-run", action="store_true",
                    help="no GPU: gloo ranks run a small CPU step through the same launch / barrier / report path")
    ap.add_argument("--enhance", action="store_true",
                    help="the enhancer stage as the headline: CLAHE-in-Lab + multi-scale factor/clamp over a resident "
                         "bs=32 512x512 batch (adaptive_params.py:121-169, multi_scale.py:62-100)")
    ap.add_argument("--detail", default=os.path.join("gpurun_out", "bench_detail.json"),
                    help="where rank 0 writes the full JSON record (per-pass tables, slowest calls, CPU details); "
                         "stdout gets the compact line ('' = no file)")
    ap.add_argument("--cpu-enhance-child", nargs=2, type=int, metavar=("N", "SIZE"), default=None,
                    help=argparse.SUPPRESS)  # internal: the enhancer CPU baseline's child process
    ap.add_argument("--amp", action="store_true",
                    help="with --train: the reference's AMP branch (autocast fp16 convs + GradScaler)")
    ap.add_argument("--full", action="store_true",
                    help="everything besides the headline: the rocprofv3 PMC traffic passes, the nested "
                         "fp16_preact_aspp / enhance / train_amp objects, parity against the CPU oracle, the CPU "
                         "baselines and the training leg's extra profiled step (--no-traffic, --no-nested and "
                         "--cpu-seconds 0 trim it).  Without it a run sets up, warms up, times the steps and prints "
                         "the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps rank 0 writes what the last timed step returned as DIR/<name>.npy "
                         "(float32; outputs over 16 MiB as a fixed seeded sample of their elements)")
    args = ap.parse_args(argv)
    if not args.full:  # a plain run: the headline only
        args.no_traffic = True
        args.no_nested = True
        args.cpu_seconds = 0.0
    return args


# ----------------------------------------------------------------------------
# --dump-outputs: what the timed path returned in its last step
# ----------------------------------------------------------------------------
DUMP_MAX_ELEMS = 4 << 20  # per array: 16 MiB of float32 (at most three arrays per headline: 48 MiB)
DUMP_SEED = 20240229


def dump_outputs(dirname, named):
    """Write each (name, tensor) as dirname/name.npy in float32 (float64 stays
    float64).  An array of more than DUMP_MAX_ELEMS elements is written as a
    1-D sample: the elements at DUMP_MAX_ELEMS flat (C-order) indices drawn
    with replacement by a CPU generator seeded with DUMP_SEED, in ascending
    order; the indices depend on the element count alone, so two builds run
    with the same arguments write the same elements."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    for name, t in named:
        t = torch.as_tensor(t).detach()
        t = t.to(torch.float64 if t.dtype == torch.float64 else torch.float32).contiguous()
        if t.numel() > DUMP_MAX_ELEMS:
            g = torch.Generator().manual_seed(DUMP_SEED)
            idx = torch.randint(0, t.numel(), (DUMP_MAX_ELEMS,), generator=g).sort().values
            t = t.reshape(-1)[idx.to(t.device)]
        np.save(os.path.join(dirname, name + ".npy"), t.cpu().numpy())


# ----------------------------------------------------------------------------
# host CPU description and the CPU baselines (oracle = checker / baseline only)
# ----------------------------------------------------------------------------
def cpu_info():
    """Cores this process may use: the affinity mask, capped by a cgroup CPU
    quota when one is set (on the GPU box os.cpu_count() reports the whole
    machine while the job's share is far smaller; threads beyond the share
    only oversubscribe it)."""
    total = os.cpu_count() or 1
    try:
        aff = len(os.sched_getaffinity(0))
    except AttributeError:
        aff = total
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
            if q != "max":
                quota = float(q) / float(per)
    except (OSError, ValueError):
        pass
    usable = aff if quota is None else max(1, min(aff, int(quota + 0.5)))
    model = None
    try:
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.startswith("model name"):
                    model = ln.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return {"threads": usable, "os_cpu_count": total, "affinity": aff, "cgroup_quota_cpus": quota,
            "cpu_model": model}


def _median_reps(fn, reps=CPU_REPS):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    times.sort()
    return times[len(times) // 2], times


def cpu_baseline(sd, pre, aspp, size, sample, note):
    """oracle/net.py forward (torch-CPU fp32) on `sample` images: 1 warm-up
    image, then the median of CPU_REPS timed forwards of the whole sample."""
    from oracle import net as onet  # checker / baseline only
    ci = cpu_info()
    torch.set_num_threads(ci["threads"])
    x1 = torch.rand(1, 3, size, size, generator=torch.Generator().manual_seed(99))
    xb = torch.rand(sample, 3, size, size, generator=torch.Generator().manual_seed(99))
    with torch.no_grad():
        onet.forward(sd, x1, pre, aspp)  # warm-up
        med, times = _median_reps(lambda: onet.forward(sd, xb, pre, aspp))
    return {"value": sample / med, "unit": "images/s", "cores": ci["threads"], "kind": "port",
            "cpu": ci, "rep_seconds": times,
            "sample": f"{sample}x3x{size}x{size} fp32 forward of oracle/net.py (torch-CPU, {note}); "
                      f"1-image warm-up, median of {CPU_REPS}"}


def cpu_train_baseline(sd, size, batch=8):
    """oracle/train.py step (torch-CPU fp32 autograd) on the configs[4] batch of
    `batch` images (BatchNorm couples the images, so the batch is the unit:
    SURVEY §8(d) "C5 at bs=8"): 1 warm-up step on one image, then the median
    of 2 timed steps of the whole batch (~15 s each on 16 cores)."""
    from oracle import train as otrain  # checker / baseline only
    ci = cpu_info()
    torch.set_num_threads(ci["threads"])
    vgg = otrain.vgg19_state(1234)
    x1 = torch.rand(1, 3, size, size, generator=torch.Generator().manual_seed(98))
    xb = torch.rand(batch, 3, size, size, generator=torch.Generator().manual_seed(98))

    def one(x):
        otrain.train_step({k: v.clone() for k, v in sd.items()}, vgg, x, False, False)
    one(x1)
    med, times = _median_reps(lambda: one(xb), reps=2)
    return {"value": batch / med, "unit": "images/s", "cores": ci["threads"], "kind": "port",
            "cpu": ci, "rep_seconds": times,
            "sample": f"{batch}x3x{size}x{size} training step of oracle/train.py (torch-CPU autograd, fp32; "
                      f"the configs[4] batch); 1-image warm-up step, median of 2"}


def parity_vs_cpu(sd, pre, aspp, x, outs, precision):
    """Per-pixel max |d| of images 0 and B-1 of the last timed step's outputs
    (the first and last image of the shard, as the GPU tests check) against
    the CPU oracle (oracle/net.py, fp32) on the same inputs (the fp16 run's
    input is the fp16-rounded image, widened to fp32 for the oracle)."""
    from oracle import net as onet  # checker only
    idx = [0] if x.shape[0] == 1 else [0, x.shape[0] - 1]
    with torch.no_grad():
        ref = onet.forward(sd, x[idx].float().cpu(), pre, aspp)
    names = ("enhanced", "reflectance", "illumination")
    d = {n: (o[idx].float().cpu() - r).abs().max().item() for n, o, r in zip(names, outs, ref)}
    if precision == "fp16":  # reflectance x/(I+1e-6) is unbounded: relative to max(1, max|R|) as in the tests
        d["reflectance"] /= max(1.0, ref[1].abs().max().item())
    tol = 1e-3  # fp32: north_star; fp16: tests/test_gpu_bn_parity.py FP16_TOL
    return {"max_abs_diff": d, "tol": tol, "pass": all(v <= tol for v in d.values()), "images": idx,
            "sample": f"images {idx} of rank 0's last timed batch vs oracle/net.py fp32 on host cores"}


# ----------------------------------------------------------------------------
# PMC traffic (child passes before this process touches the GPU)
# ----------------------------------------------------------------------------
# every kernel launch_conv dispatches to (the bench's conv family = the executor's GEMM ops)
CONV_KERNELS = ("conv_halo_kernel", "conv_igemm_kernel", "conv_wide_kernel", "conv_wide32_kernel",
                "conv_ring_kernel", "conv_ring32_kernel", "conv_hwide_kernel", "conv_hwide3_kernel",
                "conv_hwide4_kernel", "conv_t2_kernel", "conv_t2_f32_kernel")


def pmc_traffic(precision, variant, batch, size, extra=(), kernels=CONV_KERNELS):
    """HBM bytes of the conv kernels per forward from rocprofv3 PMC counters.

    Two child passes of this script (one forward of warm-up + one timed) under
    `rocprofv3 --pmc FETCH_SIZE` and `--pmc WRITE_SIZE` (separate passes: they
    do not fit one pass on gfx950).  FETCH_SIZE (KB) reports half the bytes of
    wide coalesced reads on gfx950, so it is doubled (MI355X_MICROARCH.md, HBM
    section).  Returns None on failure."""
    import csv
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3")
    if exe is None:
        return None
    out = {}
    base = [sys.executable, os.path.abspath(__file__), "--steps", "1", "--warmup", "1", "--cpu-seconds", "0",
            "--no-profile", "--no-traffic", "--no-nested", "--detail", "", "--batch", str(batch), "--size", str(size),
            "--precision", precision, "--variant", variant] + list(extra)
    env = dict(os.environ, TMPDIR="/tmp")
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="upr_pmc_", dir="/tmp")
        cmd = [exe, "--pmc", ctr, "--kernel-trace", "-T", "-d", d, "-o", "p", "--output-format", "csv", "--"] + base
        try:
            subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                           timeout=300, check=True)
            path = None
            for root, _, files in os.walk(d):
                for f in files:
                    if f.endswith("counter_collection.csv"):
                        path = os.path.join(root, f)
            if path is None:
                return None
            tot, n = 0.0, 0
            with open(path) as f:
                for r in csv.DictReader(f):
                    if r["Counter_Name"] == ctr and any(k in r["Kernel_Name"] for k in kernels):
                        tot += float(r["Counter_Value"])
                        n += 1
            out[ctr] = (tot, n)
        except Exception:
            return None
        finally:
            shutil.rmtree(d, ignore_errors=True)
    fetch_kb, n_launch = out["FETCH_SIZE"]
    write_kb, _ = out["WRITE_SIZE"]
    if n_launch == 0:
        return None
    per_fwd = (2.0 * fetch_kb + write_kb) * 1024.0 / 2.0  # 2 forwards (1 warm-up + 1 timed)
    return {"bytes_per_launch": per_fwd / (n_launch / 2.0), "bytes_per_forward": per_fwd,
            "read_bytes_per_forward": 2.0 * fetch_kb * 1024.0 / 2.0, "write_bytes_per_forward": write_kb * 1024.0 / 2.0,
            "launches_per_forward": n_launch / 2.0}


# ----------------------------------------------------------------------------
# ranks
# ----------------------------------------------------------------------------
def launch_ranks(args):
    """`--gpus N` without WORLD_SIZE: this process is only the launcher and never
    initialises the GPU.  It runs torch.distributed.run with N ranks (one per
    GPU, rendezvous on 127.0.0.1) over this same script and exits with its code;
    rank 0 prints the JSON line."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", f"--master-port={port}", os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    return subprocess.call(cmd, env=env)


def dist_setup(args):
    """(world, rank, device) of this process; initialises the process group
    (RCCL over xGMI on the GPU, gloo for --dry-run) when WORLD_SIZE > 1."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.dry_run:
        if world > 1:
            torch.distributed.init_process_group("gloo")
        return world, rank, torch.device("cpu")
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    if world > 1:
        torch.distributed.init_process_group("nccl", device_id=dev)
    return world, rank, dev


def sync(world, dev):
    if world > 1:
        torch.distributed.barrier()
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)


def max_over_ranks(world, dev, seconds):
    if world == 1:
        return seconds
    t = torch.tensor([seconds], device=dev, dtype=torch.float64)
    torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
    return t.item()


def timed_loop(world, dev, steps, warmup, step, profile_last=None):
    """warmup untimed steps, then `steps` timed ones bracketed by barrier +
    synchronize; returns (max-over-ranks seconds, last step's result).
    profile_last(True) is called before the LAST timed step (per-launch
    events); the caller reads and disables the profile."""
    for _ in range(warmup):
        step()
    sync(world, dev)
    last = None
    t0 = time.perf_counter()
    for i in range(steps):
        if profile_last is not None and i == steps - 1:
            profile_last(True)
        last = step()
    sync(world, dev)
    el = time.perf_counter() - t0
    return max_over_ranks(world, dev, el), last


def collect_fn(mode, world):
    if mode == "none" or world == 1:  # one rank: nothing to collect
        return None
    from upr.dist import gather_shards, gather_to_rank0
    return gather_shards if mode == "all" else gather_to_rank0


# ----------------------------------------------------------------------------
# forward leg (configs[1] / [2] / [3])
# ----------------------------------------------------------------------------
def cfg_label(precision, variant, size, batch):
    """The BASELINE.json configs[] entry a forward run IS, or "off-config".

    configs[1]: bs=32 512^2 random-init forward, fp32 (the plain model, the
                reference's default UP_Retinex flags in bench terms);
    configs[2]: bs=32 512^2 fp16 with ASPP + preact;
    configs[3]: bs=256 1024^2 over 8 GPUs, i.e. 32 images of 1024^2 per GPU,
                preact + ASPP (the UP_Retinex() default of enhance_batch_images),
                fp32 or fp16 (BASELINE.json names no precision).
    Anything else (fp16 plain, fp32 preact+ASPP at 512^2, other batch sizes)
    is a number on a config BASELINE.json does not define."""
    if batch == 32 and size == 512 and precision == "fp32" and variant == "plain":
        return "configs[1]"
    if batch == 32 and size == 512 and precision == "fp16" and variant == "preact_aspp":
        return "configs[2]"
    if batch == 32 and size == 1024 and variant == "preact_aspp":
        return "configs[3]"
    return "off-config"


def conv_roofline(stats, precision, B, traffic):
    gemm = [s for s in stats if s["kind"] == "conv_igemm"]
    g_ms = sum(s["ms"] for s in gemm)
    g_calls = sum(s["calls"] for s in gemm)
    g_flops = sum(s["flops"] for s in gemm)
    g_bytes = sum(s["bytes"] for s in gemm)
    all_ms = sum(s["ms"] for s in stats)
    achieved = g_flops / (g_ms * 1e-3) / 1e12 if g_ms > 0 else 0.0
    peak = PEAK_TFLOPS[precision]
    # per-layer roofline: each conv launch is bounded by max(flops / MFMA
    # peak, algorithmic bytes / HBM peak); layer_frac = sum of those bounds
    # over the measured conv time (1.0 = every conv at its own roofline)
    t_roof = sum(max(s["flops"] / (peak * 1e12), s["bytes"] / (PEAK_HBM_GBS * 1e9)) for s in gemm)
    n_hbm = sum(1 for s in gemm if s["bytes"] / (PEAK_HBM_GBS * 1e9) > s["flops"] / (peak * 1e12))
    # the MFMA-bound 3x3 convs on their own (north_star: >= 0.6 of the fp16 MFMA roofline on the 3x3 hot path)
    mf = [s for s in gemm if s["flops"] / (peak * 1e12) >= s["bytes"] / (PEAK_HBM_GBS * 1e9)]
    mf_ms = sum(s["ms"] for s in mf)
    mf_fl = sum(s["flops"] for s in mf)
    return {
        "bound": "mfma", "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
        "traffic": traffic["bytes_per_launch"] if traffic else None,
        "traffic_unit": "bytes per conv launch (rocprofv3 FETCH_SIZE*2 + WRITE_SIZE; N=1 only, per rank)",
        "traffic_per_img_GB": traffic["bytes_per_forward"] / B / 1e9 if traffic else None,
        "alg_bytes_per_launch": g_bytes / max(g_calls, 1),
        "kernel": "conv family: " + "/".join(k[:-7] for k in CONV_KERNELS) + " (all conv launches of the step)",
        "profiled_steps": 1,
        "launches_per_step": g_calls,
        "avg_launch_us": 1000.0 * g_ms / max(g_calls, 1),
        "gemm_gflop_per_img": g_flops / B / 1e9,
        "gemm_alg_GB_per_img": g_bytes / B / 1e9,
        "gemm_share_of_device_time": g_ms / all_ms if all_ms else None,
        "layer_roofline_frac": (t_roof * 1e3) / g_ms if g_ms > 0 else None,
        "layer_roofline_note": f"sum over conv launches of max(flops/MFMA peak, alg bytes/HBM peak) / measured; "
                               f"{n_hbm} of {len(gemm)} conv ops are HBM-bound at {precision}",
        "mfma_bound_layers": {"launches": len(mf), "ms": mf_ms,
                              "achieved_TFLOPs": mf_fl / (mf_ms * 1e-3) / 1e12 if mf_ms > 0 else None,
                              "frac": mf_fl / (mf_ms * 1e-3) / 1e12 / peak if mf_ms > 0 else None},
    }


def forward_leg(args, world, rank, dev, precision, variant, B, S, traffic, cpu_sample, dump=None):
    """One forward config: build the seeded model, time `args.steps` forwards of
    this rank's resident shard, report the roofline and, with --full, parity and
    the CPU baseline; `dump` is the --dump-outputs directory of the headline leg."""
    from models.model import UP_Retinex
    pre = aspp = variant == "preact_aspp"
    torch.manual_seed(0)
    model = UP_Retinex(use_preact=pre, use_aspp=aspp).eval()
    sd_cpu = {k: v.clone() for k, v in model.state_dict().items()}
    dt = torch.float16 if precision == "fp16" else torch.float32
    model = model.to(dev)
    if precision == "fp16":
        model = model.half()
    x = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(1 + rank)).to(dev, dt)
    collect = collect_fn(args.collect, world)

    def step():
        with torch.no_grad():
            out = model(x)
            if collect is not None:  # SURVEY §8e final collect: fp16 enhanced images
                collect(out[0].half(), world * B)
            return out

    step()  # first warm-up step: builds the executor handle
    torch.cuda.synchronize()
    handle = next(iter(model.__dict__["_upr_cache"].values()))[1]
    # per-launch HIP events in the LAST timed step only: events around every
    # launch of every step cost ~5% of the fp16 step (two event packets per launch)
    prof = None if args.no_profile else handle.profile
    elapsed, last = timed_loop(world, dev, args.steps, max(args.warmup - 1, 0), step, prof)
    stats = handle.profile_read() if not args.no_profile else []
    handle.profile(False)
    total = world * B * args.steps
    out = {
        "metric": f"images/sec at {S}x{S} bs={B} per GPU (UP-Retinex forward)",
        "value": total / elapsed, "unit": "images/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": 1000.0 * elapsed / args.steps, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None,
        "dtype": "f32" if precision == "fp32" else "f16 (fp32 accumulate)",
        "data": "synthetic torch.rand inputs, random-init weights (torch.manual_seed(0))",
        "config": {"workload": f"{cfg_label(precision, variant, S, B)}: bs={B}/GPU {S}x{S} "
                               f"{variant} forward, {precision}",
                   "global_batch": world * B, "image_size": S, "variant": variant,
                   "parallelism": f"batch-shard x{world} " + {
                       "none": "(no data-path collective)",
                       "all": "(+ timed final collect: RCCL all_gather_into_tensor of fp16 enhanced to every rank)",
                       "rank0": "(+ timed final collect: RCCL gather of fp16 enhanced to rank 0)"}[args.collect]},
    }
    # which executor ran the timed steps: the library counts the forwards that
    # forked the multi-scale side stream (csrc/model.hip side_of); the profiled
    # last step always stays on one stream
    forked = handle.forks()
    two = forked >= args.steps + max(args.warmup - 1, 0)
    out["executor"] = ("two streams: the multi-scale ops on a side stream forked before the bottleneck, joined "
                       "before the Retinex tail (DESIGN §3)" if two else "one stream") + \
        f" ({forked} of {args.steps + args.warmup} forwards forked)" + \
        ("; roofline per-launch events from the serialised profiled step" if stats else "")
    if stats:
        rf = conv_roofline(stats, precision, B, traffic)
        rf["ref_equiv_tflops"] = REF_GFLOP_PER_IMG[variant] * (S / 512) ** 2 * total / world / elapsed / 1e3
        if args.ceilings:
            from upr.calib import measure
            cz = measure(dev)
            mf = cz["mfma_f16_TF"] if precision == "fp16" else 155.0  # fp32: MI355X_MICROARCH.md measured
            hb = max(cz["hbm_copy_TBps"] * 1e3, 6290.0)
            gemm = [s for s in stats if s["kind"] == "conv_igemm"]
            g_ms = sum(s["ms"] for s in gemm)
            t_meas = sum(max(s["flops"] / (mf * 1e12), s["bytes"] / (hb * 1e9)) for s in gemm)
            rf["measured_ceilings"] = {
                "mfma_TFLOPs": mf, "hbm_GBs": hb, "detail": cz, "frac_vs_measured_mfma": rf["achieved"] / mf,
                "layer_roofline_frac_vs_measured": (t_meas * 1e3) / g_ms if g_ms > 0 else None,
                "note": "fp16: best of 1/2 waves per SIMD of back-to-back 16x16x32 MFMAs on random register "
                        "operands after 2 s of load; HBM: max(this run's best 16-B/lane copy of 1 GiB, "
                        "MI355X_MICROARCH.md's measured 6.29 TB/s float4 copy)"}
        out["roofline"] = rf
        if args.breakdown and rank == 0:
            for s in stats:
                tf = s["flops"] / (s["ms"] * 1e-3) / 1e12 if s["ms"] else 0
                gbs = s["bytes"] / (s["ms"] * 1e-3) / 1e9 if s["ms"] else 0
                print(f"{s['name']:44s} {s['kind']:10s} {s['ms'] / max(s['calls'], 1):9.3f} ms "
                      f"{tf:8.1f} TF/s {gbs:8.1f} GB/s", file=sys.stderr)
    if rank == 0 and dump:
        dump_outputs(dump, zip(("enhanced", "reflectance", "illumination"), last))
    if rank == 0 and args.full:
        out["parity"] = parity_vs_cpu(sd_cpu, pre, aspp, x, last, precision)
        if world == 1 and args.cpu_seconds > 0 and cpu_sample:
            n, note = cpu_sample
            out["cpu_baseline"] = cpu_baseline(sd_cpu, pre, aspp, S, n, note)
    del model, x, last
    torch.cuda.empty_cache()
    return out


# ----------------------------------------------------------------------------
# training leg (configs[4])
# ----------------------------------------------------------------------------
def train_parity(sd, x, d0, amp, pre=False, aspp=False):
    """The first step's loss terms (initial weights, train-mode BatchNorm over
    the batch) against oracle/train.py's forward + TotalLoss (fp32 torch-CPU)
    on the same images.  BatchNorm couples the images, so the oracle runs the
    whole batch (forward and loss only, no backward).  The ASPP variant's
    train-mode Dropout draws a device mask the oracle would need replayed
    (tests/test_gpu_train.py does that): not checked here."""
    if aspp:
        return {"pass": None, "sample": "not checked: the ASPP variant's train-mode Dropout mask (the gradient "
                                        "tests replay it, tests/test_gpu_train.py::test_train_grads_variants_vs_oracle)"}
    from oracle import net as onet  # checker only
    from oracle import train as otrain
    work = {k: v.clone() for k, v in sd.items()}
    with torch.no_grad(), otrain.train_mode():
        e, r, i = onet.forward(work, x.float().cpu(), pre, False)
        _, dr = otrain.total_loss(otrain.vgg19_state(1234), x.float().cpu(), e, i, r)
    keys = ("total", "exposure", "smoothness", "color", "spatial", "decouple", "perceptual", "frequency")
    rel = {k: abs(d0[k] - dr[k]) / max(abs(dr[k]), 1e-12) for k in keys if k in d0 and k in dr}
    tol = 1e-2 if amp else 1e-4  # tests/test_gpu_train.py::test_train_step_full_size_bs8_512
    return {"rel_diff": rel, "tol": tol, "pass": all(v <= tol for v in rel.values()),
            "sample": f"loss terms of the first step (initial weights) over rank 0's whole {x.shape[0]}-image batch "
                      f"vs oracle/train.py forward + TotalLoss (fp32 torch-CPU, train-mode BatchNorm)"}


def call_bound(kind, what, fl, ms, sh, B):
    """The roofline bound of one timed training conv call (see bound_note)."""
    if not sh or ms <= 0:
        return {}
    ci, co, k, s, H, W = sh
    ho, wo = H // s, W // s
    xb, yb = 2.0 * B * H * W * ci, 2.0 * B * ho * wo * co
    nbytes = xb + yb + 2.0 * ci * co * k * k
    peak = PEAK_TFLOPS["fp16"] if kind == "mfma16" else PEAK_TFLOPS["fp32"]
    bound = max(fl / 1e9 / peak, nbytes / 1e6 / PEAK_HBM_GBS)  # ms
    return {"bound_ms": round(bound, 4), "x_bound": round(ms / bound, 2)}


def train_roofline(recs, step_ms, B, S):
    """Convs of the profiled step against the peak of the arithmetic they ran
    in (fp16 MFMA under autocast, fp32 MFMA otherwise); the rest of the step
    (BatchNorm, ReLU masks, casts, losses, FFTs, clip + Adam: fp32, memory
    bound) is reported as its time, not against an MFMA peak."""
    by = {}
    for kind, what, fl, ms, *_ in recs:
        d = by.setdefault(kind, {"ms": 0.0, "gflop": 0.0, "calls": 0})
        d["ms"] += ms
        d["gflop"] += fl / 1e9
        d["calls"] += 1
    by_what = {}
    for kind, what, fl, ms, *_ in recs:
        d = by_what.setdefault(f"{kind}.{what}", {"ms": 0.0, "gflop": 0.0, "calls": 0})
        d["ms"] += ms
        d["gflop"] += fl / 1e9
        d["calls"] += 1
    for d in by_what.values():
        d["TFLOPs"] = d["gflop"] / d["ms"] if d["ms"] > 0 else None
    for k, d in by.items():
        d["TFLOPs"] = d["gflop"] / d["ms"] if d["ms"] > 0 else None  # GF / ms = TF/s
        d["peak"] = PEAK_TFLOPS["fp16"] if k == "mfma16" else PEAK_TFLOPS["fp32"]
        d["frac"] = d["TFLOPs"] / d["peak"] if d["TFLOPs"] else None
    main = "mfma16" if "mfma16" in by else "mfma32"
    conv_ms = sum(d["ms"] for d in by.values())
    m = by.get(main, {"ms": 0.0, "gflop": 0.0})
    ach = m["gflop"] / m["ms"] if m["ms"] else 0.0
    peak = PEAK_TFLOPS["fp16" if main == "mfma16" else "fp32"]
    return {"bound": "mfma", "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak, "traffic": None,
            "kernel": f"{main} conv calls of one profiled step (forward, input gradient, weight gradient; each call "
                      f"timed with HIP events around its library call(s), algorithmic flops)",
            "by_arithmetic": by, "by_pass": by_what,
            "slowest_calls": [dict({"kind": k, "pass": w, "shape": ("%d->%d k%d s%d %dx%d" % sh) if sh else None,
                                    "ms": round(ms, 4), "TFLOPs": round(fl / 1e9 / ms, 1) if ms > 0 else None},
                                   **call_bound(k, w, fl, ms, sh, B))
                              for k, w, fl, ms, sh in sorted(recs, key=lambda r: -r[3])[:16]],
            "bound_note": "bound_ms per call = max(algorithmic flops / the arithmetic's peak, the minimal operand "
                          "bytes / 8 TB/s) with fp16 tensors in and out (fwd: x + y, dgrad: dy + dx, wgrad: x + dy; "
                          "the step also writes fp32 copies where its fp32 BatchNorm / loss read them); x_bound = "
                          "ms / bound_ms",
            "step_ms": step_ms, "conv_ms": conv_ms,
            "non_conv_ms": step_ms - conv_ms,
            "non_conv_note": "BatchNorm stats/apply, ReLU masks, fp32<->fp16 casts, pooling, losses, FFTs, "
                             "clip + Adam: fp32 memory-bound passes, not priced against an MFMA peak",
            "whole_step_TFLOPs": TRAIN_GFLOP_PER_IMG * (S / 512.0) ** 2 * B / step_ms,
            "whole_step_frac_fp16_peak": TRAIN_GFLOP_PER_IMG * (S / 512.0) ** 2 * B / step_ms / PEAK_TFLOPS["fp16"]}


def train_leg(args, world, rank, dev, B, S, amp, steps, warmup, variant, dump=None):
    from models.model import UP_Retinex
    from losses.loss import TotalLoss
    from trainers.train import make_optimizer, train_step
    from upr import train as T
    torch.manual_seed(0)
    model = UP_Retinex(use_preact=variant == "preact_aspp", use_aspp=variant == "preact_aspp")
    sd_cpu = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(dev).train()
    crit = TotalLoss(use_freq_loss=True).to(dev)
    opt = make_optimizer(model, lr=1e-4, weight_decay=1e-5)
    x = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(2 + rank)).to(dev)
    from upr.dist import allreduce_grads
    scaler = None
    if amp:
        from trainers.train import GradScaler
        scaler = GradScaler()

    def tstep():
        hook = (lambda: allreduce_grads(opt)) if world > 1 else None
        return train_step(model, x, crit, opt, scaler=scaler, use_amp=amp, grad_hook=hook)

    _, d0 = tstep()  # first warm-up step: its loss dict (initial weights) is the parity sample
    elapsed, last = timed_loop(world, dev, steps, max(warmup - 1, 0), tstep)
    if rank == 0 and dump:
        # what the step's caller holds afterwards: the loss, its terms (sorted by name) and the updated parameters
        terms = sorted((k, float(v)) for k, v in last[1].items() if isinstance(v, (int, float)))
        dump_outputs(dump, [("loss", torch.tensor([float(last[0])], dtype=torch.float64)),
                            ("loss_terms", torch.tensor([v for _, v in terms], dtype=torch.float64)),
                            ("parameters", torch.cat([p.detach().reshape(-1).float() for p in model.parameters()]))])
    step_ms = 1000.0 * elapsed / steps
    recs, prof_ms = None, None
    if args.full:
        # one more (untimed) step with per-conv HIP events for the roofline split
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        T.profile_begin()
        tstep()
        recs = T.profile_end()
        prof_ms = 1000.0 * (time.perf_counter() - t0)
    imgs = world * B * steps
    out = {
        "metric": f"train images/sec at {S}x{S} bs={B} (UP-Retinex fwd + TotalLoss + bwd + clip + Adam)",
        "value": imgs / elapsed, "unit": "images/s", "n_gpus": world, "steps": steps,
        "warmup": warmup, "ms_per_step": step_ms, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None,
        "dtype": "f16 convs under autocast (fp32 accumulate; fp16-operand weight gradients; fp32 BN / loss / Adam)"
                 if amp else "f32",
        "data": "synthetic torch.rand inputs, random-init weights (seed 0), seeded random-init VGG19 (seed 1234)",
        "config": {"workload": f"configs[4]: bs={B}/GPU {S}x{S} {variant} train step"
                               + (" AMP: autocast (fp16 MFMA convs) + GradScaler" if amp else " (fp32)"),
                   "global_batch": world * B, "image_size": S, "variant": variant,
                   "parallelism": f"data-parallel x{world} (per-rank shard"
                                  + (", RCCL all-reduce of the flat gradient buffer)" if world > 1 else ")")},
        "last_loss": last[1] if last is not None else None,
    }
    if recs is not None:
        out["roofline"] = train_roofline(recs, step_ms, B, S)
        out["profiled_step_wall_ms"] = prof_ms
    if rank == 0 and args.full:
        out["parity"] = train_parity(sd_cpu, x, d0, amp, variant == "preact_aspp", variant == "preact_aspp")
        if world == 1 and args.cpu_seconds > 0:
            out["cpu_baseline"] = cpu_train_baseline(sd_cpu, S)
    del model, x, opt, crit
    torch.cuda.empty_cache()
    return out


# ----------------------------------------------------------------------------
# enhancer leg (what main.py --mode enhance runs after the model: SURVEY §8a a11-a16)
# ----------------------------------------------------------------------------
# the CLAHE-in-Lab pipeline's kernels (one upr_clahe_enhance call) and the multi-scale ones
CLAHE_KERNELS = ("clahe_hist_kernel", "clahe_lut_kernel", "clahe_apply_kernel")
MS_KERNELS = ("ms_rows1_kernel", "ms_rows_kernel", "ms_sums3_kernel", "ms_fin1_kernel", "ms_fin_kernel",
              "scale_clamp_kernel")


_ENH_DATA = {}


def _enh_one(b):
    from oracle import enhancers as oenh  # checker / baseline only
    x, enh = _ENH_DATA["x"], _ENH_DATA["enh"]
    oenh.clahe_enhancement(enh[b:b + 1])
    fac = oenh.multiscale_factor(x[b:b + 1])
    torch.clamp(enh[b] * fac[0], 0, 1)


def cpu_enhance_baseline(n, size):
    """oracle/enhancers.py (numpy restatement of OpenCV's 8-bit Lab + CLAHE,
    torch-CPU multi-scale features) over all n images, one image per task on a
    pool of worker PROCESSES, one per usable core (the restatement is
    GIL-bound: threads do not scale).  Runs in a child of bench.py started
    before the parent touches the GPU (cpu_enhance_child), so the fork is of a
    process without a GPU context.  1 warm-up pass (one image per worker), then
    the median of CPU_REPS timed passes over the n images."""
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    ci = cpu_info()
    workers = max(1, min(ci["threads"], n))
    torch.set_num_threads(1)
    g = torch.Generator().manual_seed(97)
    _ENH_DATA["x"] = torch.rand(n, 3, size, size, generator=g)
    _ENH_DATA["enh"] = torch.rand(n, 3, size, size, generator=g) * 0.8
    with ProcessPoolExecutor(workers, mp_context=mp.get_context("fork")) as ex:
        list(ex.map(_enh_one, range(workers)))  # warm-up: imports + first touch in every worker
        med, times = _median_reps(lambda: list(ex.map(_enh_one, range(n))))
    return {"value": n / med, "unit": "images/s", "cores": workers, "kind": "port", "cpu": ci, "rep_seconds": times,
            "sample": f"{n}x3x{size}x{size}: oracle/enhancers.py clahe_enhancement (numpy OpenCV restatement) + "
                      f"multiscale_factor + clamp, one image per task on {workers} worker processes; warm-up pass, "
                      f"median of {CPU_REPS}"}


def _under_profiler():
    """True under rocprofv3 (its preloaded library initialises the GPU before
    main()): the child-process legs -- PMC passes, the forked CPU enhancer
    pool -- are then skipped, since a fork or exec from a GPU-initialised
    process is not allowed; their results are reported as absent."""
    return any(k.startswith("ROCPROF") for k in os.environ)


_CPU_SKIPPED = {"value": None, "unit": "images/s", "cores": 0, "kind": "port",
                "sample": "skipped: run under rocprofv3, whose preloaded library initialised the GPU before "
                          "main() (no forked CPU pool from a GPU-initialised process)"}


def cpu_enhance_child(n, size):
    """Run cpu_enhance_baseline in a child process (before this process
    initialises the GPU); None on failure."""
    import subprocess
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-enhance-child", str(n), str(size)],
                           capture_output=True, text=True, timeout=600, check=True)
        return json.loads(r.stdout.strip().splitlines()[-1])
    except Exception as e:  # reported, not fatal: the baseline is not the measurement
        return {"value": None, "error": f"{type(e).__name__}: {e}"[:300]}


def enhance_leg(args, world, rank, dev, B, S, traffic, cpu_res, dump=None):
    """One step = the enhancers over a resident batch of B SxS images: the
    CLAHE-in-Lab pipeline of apply_clahe_enhancement on the enhanced images
    (upr_clahe_enhance: quantise + Lab + tile histograms -> LUTs -> blend +
    Lab->RGB) and the multi-scale factor + clamp of apply_multi_scale_enhancement
    (upr_multiscale).  Each stage is timed with HIP events on the stream the
    library launches on (torch's current stream) in every timed step."""
    from upr import runtime
    g = torch.Generator(device=dev).manual_seed(3 + rank)
    x = torch.rand(B, 3, S, S, device=dev, generator=g)
    enh = torch.rand(B, 3, S, S, device=dev, generator=g) * 0.8  # stand-in for the model's enhanced images
    ev = []

    def step():
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        o1 = runtime.clahe_enhance(enh)
        e[1].record()
        o2, _, _ = runtime.multiscale(x, enh)
        e[2].record()
        ev.append(e)
        return o1, o2

    for _ in range(max(args.warmup, 1)):
        step()
    sync(world, dev)
    ev.clear()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = step()
    sync(world, dev)
    elapsed = max_over_ranks(world, dev, time.perf_counter() - t0)
    clahe_ms = sum(e[0].elapsed_time(e[1]) for e in ev) / len(ev)
    ms_ms = sum(e[1].elapsed_time(e[2]) for e in ev) / len(ev)
    HW = S * S
    clahe_bytes = B * (HW * 24 + 8 * 8 * 256)   # fp32 RGB in + out, the tile LUTs
    ms_bytes = B * HW * (12 + 24)               # the image read once for all three scales + the clamp pass
    clahe_gbs = clahe_bytes / (clahe_ms * 1e-3) / 1e9
    out = {
        "metric": f"enhancer images/sec at {S}x{S} bs={B} per GPU (CLAHE-in-Lab + multi-scale factor/clamp)",
        "value": world * B * args.steps / elapsed, "unit": "images/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": 1000.0 * elapsed / args.steps, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "u8 (8-bit Lab / histograms) over f32 images",
        "data": "synthetic torch.rand images (stand-in for the model's enhanced output)",
        "config": {"workload": f"enhancers of main.py --mode enhance on a resident bs={B}/GPU {S}x{S} fp32 batch "
                               f"(adaptive_params.py:121-169, multi_scale.py:62-100)",
                   "global_batch": world * B, "image_size": S, "parallelism": f"batch-shard x{world}"},
        "roofline": {
            "bound": "hbm", "achieved": clahe_gbs, "peak": PEAK_HBM_GBS, "unit": "GB/s",
            "frac": clahe_gbs / PEAK_HBM_GBS,
            "traffic": traffic["bytes_per_forward"] if traffic else None,
            "traffic_unit": "HBM bytes per upr_clahe_enhance call (all its kernel launches; rocprofv3 FETCH_SIZE*2 + "
                            "WRITE_SIZE, N=1 only)",
            "kernel": "upr_clahe_enhance: clahe_hist (+ clahe_lut when tiles are split into row bands) + clahe_apply "
                      "(one call, HIP events around it)",
            "alg_bytes": clahe_bytes, "alg_bytes_note": "24 B/px (fp32 RGB read once, written once) + 8x8x256 B LUTs "
                                                        "per image; the u8 L/A/B planes between the kernels are not "
                                                        "algorithmic",
            "avg_call_ms": clahe_ms,
            "multiscale": {"avg_call_ms": ms_ms, "alg_bytes": ms_bytes,
                           "achieved_GBs": ms_bytes / (ms_ms * 1e-3) / 1e9,
                           "frac": ms_bytes / (ms_ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
                           "kernel": "upr_multiscale: ms_rows1 (one colour plane per wave, all three scales from one "
                                     "register-streamed read, fp64 per-wave partials) + ms_fin1 (adds them in order, "
                                     "writes the sums and the factor) + scale_clamp",
                           "alg_bytes_note": "12 B/px: the fp32 image read once for the three scales' sums + 24 B/px "
                                             "clamp (read enh, write out)"},
        },
    }
    if rank == 0 and dump:
        dump_outputs(dump, zip(("clahe", "multiscale"), last))
    if rank == 0 and args.full:
        # parity: images 0 and B-1 of the last step vs the restatement (bit-exact bytes expected)
        from oracle import enhancers as oenh  # checker only
        idx = [0, B - 1] if B > 1 else [0]
        ref = oenh.clahe_enhancement(enh[idx].cpu())
        d = (last[0][idx].cpu() - ref).abs().max().item()
        out["parity"] = {"max_abs_diff": {"clahe": d}, "tol": 0.0, "pass": d == 0.0, "images": idx,
                         "sample": f"CLAHE output of images {idx} of rank 0's last step vs oracle/enhancers.py "
                                   f"(numpy OpenCV restatement; bit-exact)"}
        if world == 1 and cpu_res is not None:
            out["cpu_baseline"] = cpu_res
    del x, enh, last
    torch.cuda.empty_cache()
    return out


# ----------------------------------------------------------------------------
# dry run: the same launch / rank / report path with a CPU stand-in step
# ----------------------------------------------------------------------------
def dry_run(args):
    world, rank, dev = dist_setup(args)
    torch.manual_seed(rank)
    a = [torch.rand(256, 256)]

    def step():
        a[0] = torch.tanh(a[0] @ a[0].T / 256)
        col = collect_fn(args.collect, world)
        if col is not None:
            col(a[0][:4].half(), 4 * world)
        return a[0]

    elapsed, last = timed_loop(world, dev, args.steps, args.warmup, step)
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, [("dry_run", last)])
    ranks = [None] * world
    if world > 1:
        torch.distributed.all_gather_object(ranks, (rank, os.getpid()))
    else:
        ranks = [(rank, os.getpid())]
    if rank == 0:
        stand_in = {"value": None, "note": "dry run: no GPU work"}
        wl = "configs[4]" if args.train else cfg_label(args.precision, args.variant, args.size, args.batch)
        out = {"metric": "dry run (no GPU work)", "value": world * args.steps / elapsed, "unit": "steps/s",
               "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": 1000.0 * elapsed / args.steps, "ranks": ranks, "data": "none",
               "config": {"workload": wl, "parallelism": f"batch-shard x{world} collect={args.collect}"},
               "roofline": dict(stand_in, traffic=None)}
        if args.full:
            out["parity"] = dict(stand_in, max_abs_diff=None)
        if args.full and world == 1:
            out["cpu_baseline"] = dict(stand_in, cpu=cpu_info())
        if not args.no_nested and not args.train and not (args.precision == "fp16" and args.variant == "preact_aspp"):
            out["fp16_preact_aspp"] = {"value": None, "roofline": None, "parity": dict(stand_in),
                                       "config": {"workload": cfg_label("fp16", "preact_aspp", args.size, args.batch)}}
            out["enhance"] = {"value": None, "roofline": None, "parity": dict(stand_in)}
            if world == 1:
                out["train_amp"] = {"value": None, "roofline": None}
        print(json.dumps(out))
    if world > 1:
        torch.distributed.destroy_process_group()


# ----------------------------------------------------------------------------
# the printed line: compact (the driver keeps only the tail of stdout); the
# full objects (per-pass tables, slowest calls, CPU details) go to --detail
# ----------------------------------------------------------------------------
_ROOF_KEYS = ("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_per_img_GB", "gemm_alg_GB_per_img",
              "alg_bytes_per_launch", "alg_bytes", "avg_launch_us", "launches_per_step", "avg_call_ms",
              "layer_roofline_frac", "step_ms", "conv_ms", "non_conv_ms", "whole_step_frac_fp16_peak")


def _sig(v, n=5):
    if isinstance(v, float):
        return float(f"{v:.{n}g}")
    if isinstance(v, dict):
        return {k: _sig(x, n) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_sig(x, n) for x in v]
    return v


def compact(out):
    """The bench line as printed: every headline key of the contract, and per
    object only the numbers a reader checks (value, roofline frac / achieved /
    traffic, parity max and verdict, cpu_baseline value / cores / kind)."""
    c = {k: v for k, v in out.items() if not isinstance(v, dict) or k == "config"}
    if "roofline" in out and out["roofline"]:
        r = out["roofline"]
        cr = {k: r[k] for k in _ROOF_KEYS if k in r}
        if r.get("mfma_bound_layers"):
            cr["mfma_bound_layers"] = {k: r["mfma_bound_layers"].get(k) for k in ("launches", "achieved_TFLOPs", "frac")}
        if r.get("multiscale"):
            cr["multiscale"] = {k: r["multiscale"].get(k) for k in ("avg_call_ms", "achieved_GBs", "frac")}
        if r.get("measured_ceilings"):
            cr["frac_vs_measured_mfma"] = r["measured_ceilings"].get("frac_vs_measured_mfma")
        if "non_conv_ms" in r and r.get("step_ms"):
            cr["non_conv_share"] = r["non_conv_ms"] / r["step_ms"]
        xb = [c_["x_bound"] for c_ in r.get("slowest_calls") or [] if "x_bound" in c_]
        if xb:
            cr["slowest_calls_max_x_bound"] = max(xb)
        c["roofline"] = cr
    if "parity" in out and out["parity"]:
        p = out["parity"]
        c["parity"] = {k: p[k] for k in ("max_abs_diff", "rel_diff", "tol", "pass", "images") if k in p}
    if "cpu_baseline" in out and out["cpu_baseline"]:
        b = out["cpu_baseline"]
        c["cpu_baseline"] = {k: b[k] for k in ("value", "unit", "cores", "kind", "sample") if k in b}
    for k in ("fp16_preact_aspp", "enhance", "train_amp"):
        if k in out and out[k]:
            c[k] = compact(out[k])
    return _sig(c)


def emit(out, args):
    """rank 0: the full record to args.detail (when set), the compact line to stdout."""
    if args.detail:
        try:
            os.makedirs(os.path.dirname(os.path.abspath(args.detail)), exist_ok=True)
            with open(args.detail, "w") as f:
                json.dump(out, f)
            out = dict(out, detail=os.path.relpath(os.path.abspath(args.detail), REPO))
        except OSError:
            pass
    print(json.dumps(compact(out)))


# ----------------------------------------------------------------------------
def main():
    args = parse()
    if args.cpu_enhance_child:
        n, size = args.cpu_enhance_child
        print(json.dumps(cpu_enhance_baseline(n, size)))
        return
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args))
    if args.dry_run:
        return dry_run(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.enhance:
        trE = cpuE = None
        if world == 1 and not args.no_traffic and not _under_profiler():
            trE = pmc_traffic("fp32", "plain", args.batch, args.size, ["--enhance"], CLAHE_KERNELS)
        if world == 1 and args.cpu_seconds > 0:
            cpuE = cpu_enhance_child(args.batch, args.size) if not _under_profiler() else _CPU_SKIPPED
        world, rank, dev = dist_setup(args)
        out = enhance_leg(args, world, rank, dev, args.batch, args.size, trE, cpuE, args.dump_outputs)
        if rank == 0:
            emit(out, args)
        if world > 1:
            torch.distributed.destroy_process_group()
        return
    if args.train:
        world, rank, dev = dist_setup(args)
        out = train_leg(args, world, rank, dev, args.batch if args.batch != 32 else 8, args.size, args.amp,
                        args.steps, args.warmup, args.variant, args.dump_outputs)
        if rank == 0:
            emit(out, args)
        if world > 1:
            torch.distributed.destroy_process_group()
        return
    nested = not args.no_nested and not (args.precision == "fp16" and args.variant == "preact_aspp")
    traffic = traffic16 = trafficE = cpuE = None
    if world == 1 and not args.no_traffic and not _under_profiler():
        # child processes, before this process initialises the GPU
        traffic = pmc_traffic(args.precision, args.variant, args.batch, args.size)
        if nested:
            traffic16 = pmc_traffic("fp16", "preact_aspp", args.batch, args.size)
            trafficE = pmc_traffic("fp32", "plain", args.batch, args.size, ["--enhance"], CLAHE_KERNELS)
    if world == 1 and nested and args.cpu_seconds > 0:
        # a process pool: forked before any GPU context exists (not possible under a profiler)
        cpuE = cpu_enhance_child(args.batch, args.size) if not _under_profiler() else _CPU_SKIPPED
    world, rank, dev = dist_setup(args)
    B, S = args.batch, args.size
    out = forward_leg(args, world, rank, dev, args.precision, args.variant, B, S, traffic,
                      (B, "the full timed batch"), args.dump_outputs)
    if nested:
        out["fp16_preact_aspp"] = forward_leg(args, world, rank, dev, "fp16", "preact_aspp", B, S, traffic16,
                                              (B, "the full timed batch"))
        out["enhance"] = enhance_leg(args, world, rank, dev, B, S, trafficE, cpuE)
        if world == 1:
            out["train_amp"] = train_leg(args, world, rank, dev, 8, S, True, 5, 2, "plain")
    if rank == 0:
        emit(out, args)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
