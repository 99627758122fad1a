"""Batch-shard logic of upr/dist.py over a world_size-2 gloo group on CPU."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from upr.dist import shard_bounds, gather_shards, gather_to_rank0


def test_shard_bounds_cover_exactly():
    for total in (1, 7, 32, 256, 257):
        for world in (1, 2, 4, 8):
            spans = [shard_bounds(total, world, r) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == total
            assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, total, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    full = torch.arange(total * 6, dtype=torch.float32).reshape(total, 2, 3)
    a, b = shard_bounds(total, world, rank)
    got = gather_shards(full[a:b] * 1.0, total)
    ok = bool(torch.equal(got, full))
    g0 = gather_to_rank0(full[a:b] * 1.0, total)
    ok = ok and (bool(torch.equal(g0, full)) if rank == 0 else g0 is None)
    q.put((rank, ok))
    dist.destroy_process_group()


def test_gloo_gather_world2():
    ctx = mp.get_context("spawn")
    for total in (8, 5):
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_worker, args=(r, 2, port, total, q)) for r in range(2)]
        for p in procs:
            p.start()
        res = [q.get(timeout=120) for _ in procs]
        for p in procs:
            p.join(timeout=60)
        assert sorted(res) == [(0, True), (1, True)]


def _subgroup_worker(rank, world, port, total, q):
    """World 3; the subgroup is global ranks {1, 2}: its group rank 0 is global
    rank 1, so gather_to_rank0(dst=0) must land on global rank 1."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sub = dist.new_group([1, 2])  # every rank takes part in new_group
    ok = True
    if rank in (1, 2):
        full = torch.arange(total * 4, dtype=torch.float32).reshape(total, 4)
        gr = dist.get_rank(sub)
        a, b = shard_bounds(total, 2, gr)
        g0 = gather_to_rank0(full[a:b] * 1.0, total, group=sub, dst=0)
        ok = bool(torch.equal(g0, full)) if rank == 1 else g0 is None
        g1 = gather_to_rank0(full[a:b] * 1.0, total, group=sub, dst=1)
        ok = ok and (bool(torch.equal(g1, full)) if rank == 2 else g1 is None)
        got = gather_shards(full[a:b] * 1.0, total, group=sub)
        ok = ok and bool(torch.equal(got, full))
    q.put((rank, ok))
    dist.destroy_process_group()


def test_gloo_gather_subgroup_world3():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_subgroup_worker, args=(r, 3, port, 5, q)) for r in range(3)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(res) == [(0, True), (1, True), (2, True)]


def _grad_worker(rank, world, port, q):
    from types import SimpleNamespace
    from upr.dist import allreduce_grads
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    g = torch.arange(10, dtype=torch.float32) * (rank + 1)
    opt = SimpleNamespace(flat=SimpleNamespace(grad=g))
    allreduce_grads(opt)
    # mean over ranks of k * (r + 1) = k * (world + 1) / 2
    want = torch.arange(10, dtype=torch.float32) * (world + 1) / 2
    q.put((rank, bool(torch.allclose(opt.flat.grad, want))))
    dist.destroy_process_group()


def test_gloo_allreduce_grads_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_grad_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(res) == [(0, True), (1, True)]


def test_bench_gpus2_launches_two_gloo_ranks():
    """`bench.py --gpus 2` run directly is a launcher: it starts torch.distributed.run
    with 2 ranks (here with --dry-run: gloo, CPU step) and rank 0 reports
    n_gpus 2 with the max-over-ranks time; both ranks are distinct processes."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "2", "--dry-run", "--steps", "3",
                        "--warmup", "1"], capture_output=True, text=True, timeout=240, cwd=repo)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3
    ranks = out["ranks"]
    assert sorted(rk for rk, _ in ranks) == [0, 1]
    assert len({pid for _, pid in ranks}) == 2 and os.getpid() not in {pid for _, pid in ranks}


def _bench_json(args):
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py")] + args, capture_output=True, text=True,
                       timeout=240, cwd=repo)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_gpus2_line_carries_evidence_keys():
    """An N>1 line carries rank 0's parity, the roofline object and the nested
    fp16 object; cpu_baseline and train_amp are N=1 only; --collect rank0 runs
    the gather-to-rank-0 collect through the same timed loop (gloo here)."""
    out = _bench_json(["--gpus", "2", "--dry-run", "--full", "--steps", "2", "--warmup", "1", "--collect", "rank0"])
    assert out["n_gpus"] == 2
    for k in ("roofline", "parity", "fp16_preact_aspp", "config"):
        assert k in out, k
    assert "parity" in out["fp16_preact_aspp"]
    assert "cpu_baseline" not in out and "train_amp" not in out
    assert "collect=rank0" in out["config"]["parallelism"]


def test_bench_n1_line_carries_cpu_and_train_keys():
    out = _bench_json(["--dry-run", "--full", "--steps", "2", "--warmup", "1"])
    for k in ("roofline", "parity", "cpu_baseline", "fp16_preact_aspp", "train_amp"):
        assert k in out, k
    ci = out["cpu_baseline"]["cpu"]
    assert ci["threads"] >= 1 and "cpu_model" in ci and ci["os_cpu_count"] >= ci["threads"]


def test_bench_config_labels():
    """bench.py names only the configs BASELINE.json defines; every other
    combination is labelled off-config (the dry-run line carries the label)."""
    import importlib.util
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(repo, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert b.cfg_label("fp32", "plain", 512, 32) == "configs[1]"
    assert b.cfg_label("fp16", "preact_aspp", 512, 32) == "configs[2]"
    assert b.cfg_label("fp16", "preact_aspp", 1024, 32) == "configs[3]"
    assert b.cfg_label("fp32", "preact_aspp", 1024, 32) == "configs[3]"
    for args in (("fp16", "plain", 512, 32), ("fp32", "preact_aspp", 512, 32), ("fp32", "plain", 512, 8),
                 ("fp16", "preact_aspp", 512, 16), ("fp32", "plain", 1024, 32), ("fp16", "preact_aspp", 256, 32)):
        assert b.cfg_label(*args) == "off-config", args
    out = _bench_json(["--dry-run", "--full", "--steps", "1", "--warmup", "0"])
    assert out["config"]["workload"] == "configs[1]"
    assert out["fp16_preact_aspp"]["config"]["workload"] == "configs[2]"
    out = _bench_json(["--dry-run", "--steps", "1", "--warmup", "0", "--precision", "fp16"])
    assert out["config"]["workload"] == "off-config"
    out = _bench_json(["--dry-run", "--steps", "1", "--warmup", "0", "--precision", "fp16", "--variant",
                       "preact_aspp", "--size", "1024"])
    assert out["config"]["workload"] == "configs[3]" and "fp16_preact_aspp" not in out


def test_bench_plain_run_is_headline_only():
    """Without --full the line carries the headline and its roofline object and
    none of what --full adds (parity, CPU baseline, nested objects), whatever
    the trimming flags say; --steps sets the number of timed steps."""
    out = _bench_json(["--gpus", "1", "--dry-run", "--steps", "3", "--warmup", "1", "--cpu-seconds", "5"])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert "roofline" in out
    for k in ("parity", "cpu_baseline", "fp16_preact_aspp", "enhance", "train_amp"):
        assert k not in out, k


def _load_bench():
    import importlib.util
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(repo, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_bench_full_flag_gates_the_extras():
    """parse(): a plain run switches the traffic passes, the nested objects and
    the CPU baselines off; --full leaves them to their own flags."""
    b = _load_bench()
    a = b.parse(["--gpus", "1", "--steps", "4", "--warmup", "2"])
    assert not a.full and a.no_traffic and a.no_nested and a.cpu_seconds == 0 and a.dump_outputs is None
    a = b.parse(["--full"])
    assert a.full and not a.no_traffic and not a.no_nested and a.cpu_seconds > 0
    a = b.parse(["--full", "--no-nested", "--cpu-seconds", "0"])
    assert a.full and a.no_nested and a.cpu_seconds == 0 and not a.no_traffic


def test_bench_dump_outputs_small_and_sampled(tmp_path):
    """dump_outputs writes float32 .npy files: a small array whole, a large one
    as the same DUMP_MAX_ELEMS seeded flat positions on every call; float64
    stays float64."""
    import numpy as np
    b = _load_bench()
    small = torch.arange(24, dtype=torch.float16).reshape(2, 3, 4)
    big = torch.arange(b.DUMP_MAX_ELEMS + 1001, dtype=torch.float32) % 8191
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b" / "c")
    b.dump_outputs(d1, [("small", small), ("big", big), ("f64", torch.ones(3, dtype=torch.float64))])
    b.dump_outputs(d2, [("big", big + 1)])
    s = np.load(os.path.join(d1, "small.npy"))
    assert s.dtype == np.float32 and s.shape == (2, 3, 4) and np.array_equal(s, small.float().numpy())
    assert np.load(os.path.join(d1, "f64.npy")).dtype == np.float64
    g1, g2 = np.load(os.path.join(d1, "big.npy")), np.load(os.path.join(d2, "big.npy"))
    assert g1.dtype == np.float32 and g1.shape == (b.DUMP_MAX_ELEMS,) and g1.nbytes <= 16 << 20
    assert np.array_equal(g2, g1 + 1)          # the same positions both times
    assert len(np.unique(g1)) == 8191          # spread over the array, not a prefix


def test_bench_dump_outputs_same_inputs_every_run(tmp_path):
    """Two runs with the same arguments write identical arrays (the dry run's
    CPU stand-in step here; the GPU legs seed their inputs the same way)."""
    import numpy as np
    outs = []
    for name in ("r1", "r2"):
        d = str(tmp_path / name)
        _bench_json(["--gpus", "1", "--dry-run", "--steps", "2", "--warmup", "1", "--dump-outputs", d])
        assert os.listdir(d) == ["dry_run.npy"]
        outs.append(np.load(os.path.join(d, "dry_run.npy")))
    assert outs[0].dtype == np.float32 and np.array_equal(outs[0], outs[1])
