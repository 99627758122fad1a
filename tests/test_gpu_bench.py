"""bench.py on the device: a plain run's line and its --dump-outputs files
(small shapes; the headline shapes are the benchmark's own business)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]


def test_bench_plain_run_line_and_dumped_outputs(tmp_path):
    """`bench.py --gpus 1 --steps N --warmup W --dump-outputs DIR` at bs 2 40x40:
    the line carries the headline keys and none of the --full objects, N is the
    number of timed steps, and DIR holds the last step's three outputs in
    float32, which are a forward of the same seeded model on the same inputs."""
    d = str(tmp_path / "out")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--batch", "2", "--size", "40", "--detail", "", "--dump-outputs", d],
                       capture_output=True, text=True, timeout=240, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 2 and out["unit"] == "images/s" and out["higher_is_better"] is True
    assert out["dtype"] == "f32" and out["ms_per_step"] > 0
    assert abs(out["value"] - 2 * 1000.0 / out["ms_per_step"]) <= 1e-3 * out["value"]
    for k in ("parity", "cpu_baseline", "fp16_preact_aspp", "enhance", "train_amp"):
        assert k not in out, k
    assert sorted(os.listdir(d)) == ["enhanced.npy", "illumination.npy", "reflectance.npy"]

    from models.model import UP_Retinex
    torch.manual_seed(0)
    model = UP_Retinex(use_preact=False, use_aspp=False).eval().to("cuda:0")
    x = torch.rand(2, 3, 40, 40, generator=torch.Generator().manual_seed(1)).to("cuda:0")
    with torch.no_grad():
        want = model(x)
    for name, w in zip(("enhanced", "reflectance", "illumination"), want):
        got = np.load(os.path.join(d, name + ".npy"))
        assert got.dtype == np.float32 and got.shape == tuple(w.shape)
        # the same kernels on the same inputs, at most a different order of fp32 sums: a tenth of the
        # project's fp32 bound against the oracle (1e-3), relative to max(1, max|w|) since the reflectance
        # x / (I + 1e-6) is unbounded; another seed or another step's input is off by ~0.1
        w = w.float().cpu().numpy()
        err = float(np.abs(got - w).max()) / max(1.0, float(np.abs(w).max()))
        print(f"bench dump {name}: rel max|d| {err:.3e}")
        assert err <= 1e-4, name
