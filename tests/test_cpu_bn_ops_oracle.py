"""Self-check of the float64 op reference oracle/bn_ops.py (numpy) against
torch.nn.BatchNorm2d with autograd and torch.optim.Adam +
clip_grad_norm_, all in double: both sides are float64, so they agree to
1e-12 relative (of the largest reference magnitude)."""
import numpy as np
import pytest
import torch

from oracle import bn_ops as O

REL = 1e-12


def _agree(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), b.detach().double().numpy()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b).max()
    tol = REL * max(np.abs(b).max(), 1e-300)
    assert err <= tol, f"{what}: max|d| {err:.3e} > {tol:.3e}"


def _nchw(a, B, H, W):
    """[M, C] numpy -> [B, C, H, W] double tensor."""
    return torch.from_numpy(np.ascontiguousarray(a.reshape(B, H, W, -1).transpose(0, 3, 1, 2)))


def _mc(t):
    """[B, C, H, W] tensor -> [M, C] numpy."""
    return t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1]).numpy()


def _inputs(B, C, H, W, seed):
    rng = np.random.default_rng(seed)
    M = B * H * W
    x = rng.standard_normal((M, C)) * rng.uniform(0.5, 2, C) + rng.uniform(-1, 1, C)
    gamma = rng.uniform(0.5, 1.5, C) * np.where(np.arange(C) % 5 == 3, -1.0, 1.0)
    beta = rng.uniform(-0.2, 0.2, C)
    res = rng.standard_normal((M, C))
    g = rng.standard_normal((M, C))
    return M, x, gamma, beta, res, g


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("res_mode", ["none", "pre", "post"])
@pytest.mark.parametrize("B,C,H,W", [(2, 7, 5, 3), (1, 4, 1, 2)])
def test_bn_train_matches_torch_double(B, C, H, W, res_mode, relu):
    M, x, gamma, beta, res, g = _inputs(B, C, H, W, 3)
    eps, mom = 1e-5, 0.1
    bn = torch.nn.BatchNorm2d(C, eps=eps, momentum=mom).double().train()
    rm0, rv0 = np.linspace(-1, 1, C), np.linspace(0.5, 2, C)
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma))
        bn.bias.copy_(torch.from_numpy(beta))
        bn.running_mean.copy_(torch.from_numpy(rm0))
        bn.running_var.copy_(torch.from_numpy(rv0))
    xt = _nchw(x, B, H, W).requires_grad_(True)
    rt = _nchw(res, B, H, W).requires_grad_(True)
    z = bn(xt)
    pre = z + rt if res_mode == "pre" else z
    pre.retain_grad()
    yt = torch.relu(pre) if relu else pre
    if res_mode == "post":
        yt = yt + rt
    yt.backward(_nchw(g, B, H, W))

    mean, var, invstd = O.bn_stats(x, eps)
    rm, rv = O.bn_running(rm0, rv0, mean, var, M, mom)
    _agree(rm, bn.running_mean, "running_mean")
    _agree(rv, bn.running_var, "running_var")
    y = O.bn_apply(x, mean, invstd, gamma, beta, None if res_mode == "none" else res, res_mode == "post", relu)
    _agree(y, torch.from_numpy(_mc(yt)), "y")
    # the ReLU's mask is an explicit argument: the sign of the value it saw
    mask = (_mc(pre) > 0) if relu else None
    dg0, db0 = np.linspace(1, 2, C), np.linspace(-2, -1, C)
    dx, dgamma, dbeta, _ = O.bn_bwd(g, x, mean, invstd, gamma, True, mask, None, dg0, db0)
    _agree(dx, torch.from_numpy(_mc(xt.grad)), "dx")
    _agree(dgamma - dg0, bn.weight.grad, "dgamma")
    _agree(dbeta - db0, bn.bias.grad, "dbeta")
    dx0 = np.full_like(dx, 0.25)
    dxa = O.bn_bwd(g, x, mean, invstd, gamma, True, mask, dx0)[0]
    _agree(dxa - dx0, torch.from_numpy(_mc(xt.grad)), "dx accumulated")


@pytest.mark.parametrize("relu", [False, True])
def test_bn_eval_matches_torch_double(relu):
    B, C, H, W = 2, 6, 4, 3
    M, x, gamma, beta, res, g = _inputs(B, C, H, W, 4)
    eps = 1e-5
    bn = torch.nn.BatchNorm2d(C, eps=eps).double().eval()
    rm0, rv0 = np.linspace(-1, 1, C), np.linspace(0.5, 2, C)
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma))
        bn.bias.copy_(torch.from_numpy(beta))
        bn.running_mean.copy_(torch.from_numpy(rm0))
        bn.running_var.copy_(torch.from_numpy(rv0))
    xt = _nchw(x, B, H, W).requires_grad_(True)
    z = bn(xt)
    yt = torch.relu(z) if relu else z
    yt.backward(_nchw(g, B, H, W))
    mean, invstd = O.bn_eval_stats(rm0, rv0, eps)
    y = O.bn_apply(x, mean, invstd, gamma, beta, relu=relu)
    _agree(y, torch.from_numpy(_mc(yt)), "y")
    mask = (_mc(z) > 0) if relu else None
    dx, dgamma, dbeta, _ = O.bn_bwd(g, x, mean, invstd, gamma, False, mask)
    _agree(dx, torch.from_numpy(_mc(xt.grad)), "dx")
    _agree(dgamma, bn.weight.grad, "dgamma")
    _agree(dbeta, bn.bias.grad, "dbeta")
    _agree(bn.running_mean.numpy(), torch.from_numpy(rm0), "running_mean untouched")


def test_chan_sum_matches_torch_double():
    rng = np.random.default_rng(5)
    g, out0 = rng.standard_normal((37, 6)), rng.standard_normal(6)
    _agree(O.chan_sum(g), torch.from_numpy(g).sum(0), "sum")
    _agree(O.chan_sum(g, out0), torch.from_numpy(g).sum(0) + torch.from_numpy(out0), "sum accumulated")


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.8, 0.95)])
@pytest.mark.parametrize("max_norm", [None, 1.0, 1e6])
def test_adam_matches_torch_double(betas, max_norm):
    """6 steps with weight_decay > 0; the gradient scale alternates so that
    max_norm = 1 clips on some steps and not on others; 1e6 never clips;
    None takes no clip at all."""
    n, lr, eps, wd = 257, 1e-3, 1e-8, 1e-2
    rng = np.random.default_rng(6)
    p0 = rng.standard_normal(n)
    pt = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([pt], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    clipped = []
    for step in range(1, 7):
        g = rng.standard_normal(n) * (1.0 if step % 2 else 1e-2)
        pt.grad = torch.from_numpy(g.copy())
        if max_norm is not None:
            tn = torch.nn.utils.clip_grad_norm_([pt], max_norm)
        opt.step()
        p, m, v, norm = O.adam_step(p, g, m, v, step, lr, betas, eps, wd, max_norm)
        if max_norm is not None:
            _agree(norm, tn, f"norm step {step}")
            clipped.append(norm > max_norm)
        st = opt.state[pt]
        _agree(p, pt, f"p step {step}")
        _agree(m, st["exp_avg"], f"m step {step}")
        _agree(v, st["exp_avg_sq"], f"v step {step}")
    if max_norm == 1.0:
        assert any(clipped) and not all(clipped)
    if max_norm == 1e6:
        assert not any(clipped)
