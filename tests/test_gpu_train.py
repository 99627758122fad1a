"""GPU parity of the HIP training path (include/upr_train.h, upr/train.py,
upr/loss_engine.py, upr/optim.py) against the CPU oracle (oracle/train.py,
oracle/net.py in train mode) and the reference goldens G6/G7.

Tolerances (fp32 everywhere; differences are summation order only):
  * op level (conv fwd / dgrad / wgrad, BatchNorm train fwd / bwd): max |d|
    <= 1e-4 * max|ref| + 1e-6;
  * loss terms rel 1e-4, loss gradients max |d| <= 1e-4 * max|ref|;
  * full step: loss dict rel 1e-4, per-parameter gradient L2 norms rel 1e-3
    and max |d| <= 2e-3 * max|ref| (BatchNorm over B=2 at 64x64 amplifies
    reduction-order noise), parameter deltas after Adam rel 1e-3, BatchNorm
    running stats <= 1e-4.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]

DEV = "cuda"
VGG_SEED = 1234


def _close(a, b, rel, what):
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs().max().item()
    tol = rel * max(b.abs().max().item(), 1e-12) + 1e-6
    assert err <= tol, f"{what}: max|d| {err:.3e} > {tol:.3e}"


def _act(t_nhwc):
    from upr.train import Act
    return Act(t_nhwc.contiguous())


@pytest.mark.parametrize("cin,cout,k,s,p,d,bias", [
    (32, 64, 3, 2, 1, 1, False),    # encoder conv1 (stride 2)
    (64, 64, 3, 1, 1, 1, False),    # encoder conv2
    (32, 64, 1, 2, 0, 1, False),    # projecting shortcut
    (32, 32, 3, 1, 2, 2, True),     # FAM branch4_conv2 (dilation 2)
    (256, 256, 3, 1, 6, 6, False),  # ASPP d6
    (3, 32, 3, 1, 1, 1, True),      # input layer (direct)
    (32, 3, 1, 1, 0, 1, True),      # output layer (direct; coalesced 1x1 head kernel)
    (64, 1, 1, 1, 0, 1, True),      # 1x1 head, 64 channels -> 1
    (2, 1, 7, 1, 3, 1, True),       # spatial attention (direct)
])
def test_conv_layer(cin, cout, k, s, p, d, bias):
    from upr.train import Act, Conv
    torch.manual_seed(0)
    m = torch.nn.Conv2d(cin, cout, k, stride=s, padding=p, dilation=d, bias=bias)
    H = W = 16 if cin >= 256 else 24
    x = torch.randn(2, cin, H, W)
    gy_shape = m(x).shape
    gy = torch.randn(gy_shape)
    xr = x.clone().requires_grad_(True)
    y = m(xr)
    y.backward(gy)
    md = torch.nn.Conv2d(cin, cout, k, stride=s, padding=p, dilation=d, bias=bias).to(DEV)
    md.load_state_dict(m.state_dict())
    md.weight.grad = torch.zeros_like(md.weight)
    if bias:
        md.bias.grad = torch.zeros_like(md.bias)
    c = Conv(md)
    c.pack()
    xa = Act(x.permute(0, 2, 3, 1).contiguous().to(DEV))
    ya = c.fwd(xa)
    _close(ya.t.permute(0, 3, 1, 2), y, 1e-4, "fwd")
    gya = Act(gy.permute(0, 2, 3, 1).contiguous().to(DEV))
    gxa = Act.new(2, H, W, cin, DEV)
    c.bwd(xa, gya, gxa)
    torch.cuda.synchronize()
    _close(gxa.t.permute(0, 3, 1, 2), xr.grad, 1e-4, "dgrad")
    _close(md.weight.grad, m.weight.grad, 1e-4, "wgrad")
    if bias:
        _close(md.bias.grad, m.bias.grad, 1e-4, "dbias")


@pytest.mark.parametrize("nchw", [True, False])
def test_stem_relu_fused_into_wgrad(nchw):
    """Conv.bwd_relu_stem (upr_t_conv_direct_wgrad_relu: the stem's ReLU
    backward applied to dy inside the small-channel weight-gradient kernel)
    equals relu_mask + the plain direct weight gradient bit for bit, and the
    torch weight / bias gradient of relu(conv(x)) within 1e-4."""
    from upr.train import Act, Conv, nchw_view, relu_mask
    torch.manual_seed(5)
    B, H, W = 2, 40, 56
    m = torch.nn.Conv2d(3, 32, 3, padding=1)
    x = torch.rand(B, 3, H, W)
    w0 = m.weight.detach().clone()
    gy = torch.randn(B, 32, H, W)
    mr = torch.nn.Conv2d(3, 32, 3, padding=1)
    mr.load_state_dict(m.state_dict())
    torch.relu(mr(x)).backward(gy)
    outs = []
    for fused in (True, False):
        md = torch.nn.Conv2d(3, 32, 3, padding=1).to(DEV)
        md.load_state_dict(m.state_dict())
        md.weight.grad = torch.zeros_like(md.weight)
        md.bias.grad = torch.zeros_like(md.bias)
        c = Conv(md)
        c.pack()
        xd = x.to(DEV).contiguous()
        xa = Act(x.permute(0, 2, 3, 1).contiguous().to(DEV))
        if nchw:
            xv = (nchw_view(xd), B, H, W)
            y = c.fwd(None, relu=True, x_view=xv, out=Act.new(B, H, W, 32, DEV, fresh=False))
        else:
            xv = None
            y = c.fwd(xa, relu=True)
        g = Act(gy.permute(0, 2, 3, 1).contiguous().to(DEV))
        if fused:
            c.bwd_relu_stem(None if nchw else xa, g, y, x_view=xv)
        else:
            relu_mask(g, y)
            c.bwd(None if nchw else xa, g, None, x_view=xv)
        torch.cuda.synchronize()
        outs.append((md.weight.grad.clone(), md.bias.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    _close(outs[0][0], mr.weight.grad, 1e-4, "stem wgrad")
    _close(outs[0][1], mr.bias.grad, 1e-4, "stem dbias")
    assert torch.equal(m.weight.detach(), w0)


@pytest.mark.parametrize("nchw,H,W", [(True, 40, 72), (False, 24, 64), (True, 13, 7)])
def test_stem_wgrad_relu16_vs_torch(nchw, H, W):
    """upr_t_conv_stem_wgrad_relu16 (the 3 -> 32 3x3 stem weight gradient, dy
    masked by the ReLU output's fp16 copy > 0, LDS-staged tiles with ragged
    edges) vs torch's conv2d_weight of the masked dy in fp64, 1e-4 of max."""
    from upr import _lib as L
    from upr.train import nchw_view
    gen = torch.Generator().manual_seed(8)
    B = 2
    x = torch.rand(B, 3, H, W, generator=gen)
    dy = torch.randn(B, H, W, 32, generator=gen)
    y16 = torch.randn(B, H, W, 32, generator=gen).half()
    gm = dy * (y16.float() > 0)
    ref = torch.nn.grad.conv2d_weight(x.double(), (32, 3, 3, 3), gm.permute(0, 3, 1, 2).double(), padding=1).float()
    refb = gm.double().sum(dim=(0, 1, 2)).float()
    xd = x.to(DEV).contiguous()
    xn = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    xv = nchw_view(xd) if nchw else L.UprView(xn.data_ptr(), H * W * 3, W * 3, 3, 1)
    dyd, y16d = dy.to(DEV), y16.to(DEV)
    dw = torch.full((32, 3, 3, 3), 0.5, device=DEV)
    db = torch.full((32,), 0.25, device=DEV)
    rc = L.lib().upr_t_conv_stem_wgrad_relu16(ctypes.byref(xv), dyd.data_ptr(), y16d.data_ptr(), B, H, W,
                                              dw.data_ptr(), db.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    _close(dw - 0.5, ref, 1e-4, "stem wgrad")
    _close(db - 0.25, refb, 1e-4, "stem dbias")


@pytest.mark.parametrize("B,cin,cout,H,W,k,s,p,d", [
    (2, 32, 32, 64, 128, 3, 1, 1, 1),    # 32 -> 32 3x3 (dec1 / head / FAM class): BM 32, 9 runs per tile
    (1, 64, 128, 128, 128, 3, 2, 1, 1),  # encoder stride-2 conv: BM 128, 4 runs
    (1, 256, 256, 64, 64, 3, 1, 1, 1),   # bottleneck: BM 128, 72 runs (18 tiles)
    (2, 32, 64, 128, 128, 1, 2, 0, 1),   # projecting shortcut 1x1 s2: BM 64, 1 run
    (1, 32, 32, 64, 64, 3, 1, 2, 2),     # FAM branch4_conv2 (dilation 2)
    (2, 64, 64, 64, 64, 3, 1, 1, 1),     # BM 64, 9 runs x 2 tiles
    (2, 64, 32, 32, 128, 3, 1, 1, 1),    # halo form 64 -> 32 (one kernel row per block)
    (1, 32, 64, 16, 64, 3, 1, 3, 3),     # halo form 32 -> 64, dilation 3
    (1, 32, 32, 20, 64, 3, 1, 1, 1),     # H % 8 != 0: the im2col form
    (2, 96, 32, 16, 64, 1, 1, 0, 1),     # 1x1 streaming form: multi-scale head fusion 96 -> 32
    (1, 128, 32, 8, 128, 1, 1, 0, 1),    # 1x1 streaming form: FAM fusion 128 -> 32
    (1, 32, 32, 24, 24, 3, 1, 1, 1),     # Wo % 64 != 0: the fp32 path
])
def test_conv_wgrad16_vs_fp64(B, cin, cout, H, W, k, s, p, d):
    """AMP weight gradient (upr_t_conv_wgrad16): fp16-rounded operands, fp32
    accumulation -> vs the fp64 weight gradient of the same fp16-rounded x and
    dy (autocast's operands, trainers/train.py:72), max|d| <= 1e-4 max|ref|.
    Both the x16-provided and the cast-internally forms."""
    import torch.nn.functional as F
    from upr import _lib as L
    torch.manual_seed(3)
    x = torch.randn(B, cin, H, W)
    Ho = (H + 2 * p - d * (k - 1) - 1) // s + 1
    Wo = (W + 2 * p - d * (k - 1) - 1) // s + 1
    dy = torch.randn(B, cout, Ho, Wo)
    fp16_path = Wo % 64 == 0
    xh, dyh = (x.half().double(), dy.half().double()) if fp16_path else (x.double(), dy.double())
    ref = torch.nn.grad.conv2d_weight(xh, (cout, cin, k, k), dyh, stride=s, padding=p, dilation=d)
    ref = ref.permute(0, 2, 3, 1).reshape(cout, -1).float()
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    dyd = dy.permute(0, 2, 3, 1).contiguous().to(DEV)
    x16 = xd.half()
    lib = L.lib()
    st = torch.cuda.current_stream().cuda_stream
    for use_x16 in (True, False):
        dw = torch.zeros(cout, k * k * cin, device=DEV)
        rc = lib.upr_t_conv_wgrad16(xd.data_ptr(), x16.data_ptr() if use_x16 else None, B, H, W, cin, cin, 0,
                                    dyd.data_ptr(), Ho, Wo, cout, cout, 0, k, k, s, p, d, dw.data_ptr(), st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        _close(dw, ref, 1e-4, f"wgrad16 x16={use_x16}")

    # upr_t_conv_wgrad_into: the same gradient added straight into PyTorch's
    # [Co][Ci][kh][kw] layout at an unaligned offset of a flat buffer (the
    # data-parallel gradient bucket), fp16 (x16) and fp32 (no x16) arithmetic
    ref_t = ref.view(cout, k, k, cin).permute(0, 3, 1, 2).contiguous()
    ref32 = torch.nn.grad.conv2d_weight(x.double(), (cout, cin, k, k), dy.double(), stride=s, padding=p,
                                        dilation=d).float()
    for use_x16 in (True, False):
        flat = torch.zeros(cout * cin * k * k + 1, device=DEV)
        flat[0] = 7.0
        base = torch.randn(cout, cin, k, k, generator=torch.Generator().manual_seed(4))
        flat[1:] = base.reshape(-1).to(DEV)
        dy16 = dyd.half() if use_x16 else None  # the fp16 A operand as its producer would write it
        rc = lib.upr_t_conv_wgrad_into(xd.data_ptr(), x16.data_ptr() if use_x16 else None, B, H, W, cin, cin, 0,
                                       dyd.data_ptr(), dy16.data_ptr() if use_x16 else None, Ho, Wo, cout, cout, 0,
                                       k, k, s, p, d, flat.data_ptr() + 4, st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert flat[0].item() == 7.0
        want = (ref_t if use_x16 else ref32) + base
        _close(flat[1:].view(cout, cin, k, k), want, 1e-4, f"wgrad_into x16={use_x16}")


@pytest.mark.parametrize("B,C,H,W,k,s,p,nchw", [
    (2, 32, 40, 56, 3, 1, 1, False),  # EnhancedFAM branch2 max-pool (vectorised path)
    (2, 3, 64, 48, 2, 2, 0, True),    # scale2 MaxPool2d(2) on the NCHW input (scalar path)
    (1, 3, 64, 64, 4, 4, 0, True),    # scale3 MaxPool2d(4)
])
def test_maxpool_bwd_matches_torch(B, C, H, W, k, s, p, nchw):
    """upr_t_maxpool_bwd (argmax codes + deterministic gather) vs torch CPU
    max_pool2d backward, with many ties (values on a 0.25 grid: PyTorch's rule,
    the first maximal tap in window order, decides them) and one NaN window;
    dx is accumulated into (+= like the scatter form)."""
    import torch.nn.functional as F
    from upr import _lib as L
    torch.manual_seed(5)
    x = (torch.randn(B, C, H, W) * 2).round() / 4
    x[0, 0, 5, 7] = float("nan")
    xr = x.clone().requires_grad_(True)
    y = F.max_pool2d(xr, k, s, p)
    gy = torch.randn(y.shape)
    y.backward(gy)
    base = torch.randn(B, C, H, W)
    ref = xr.grad + base
    Ho, Wo = y.shape[2], y.shape[3]
    if nchw:
        xd, gyd, dxd = x.to(DEV).contiguous(), gy.to(DEV).contiguous(), base.to(DEV).contiguous()
        vx = L.UprView(xd.data_ptr(), C * H * W, W, 1, H * W)
        vg = L.UprView(gyd.data_ptr(), C * Ho * Wo, Wo, 1, Ho * Wo)
        vd = L.UprView(dxd.data_ptr(), C * H * W, W, 1, H * W)
    else:
        xd, gyd = x.permute(0, 2, 3, 1).contiguous().to(DEV), gy.permute(0, 2, 3, 1).contiguous().to(DEV)
        dxd = base.permute(0, 2, 3, 1).contiguous().to(DEV)
        vx = L.UprView(xd.data_ptr(), H * W * C, W * C, C, 1)
        vg = L.UprView(gyd.data_ptr(), Ho * Wo * C, Wo * C, C, 1)
        vd = L.UprView(dxd.data_ptr(), H * W * C, W * C, C, 1)
    import ctypes
    st = torch.cuda.current_stream().cuda_stream
    assert L.lib().upr_t_maxpool_bwd(ctypes.byref(vx), ctypes.byref(vg), B, H, W, C, k, s, p, Ho, Wo,
                                     ctypes.byref(vd), st) == 0
    torch.cuda.synchronize()
    out = dxd.cpu() if nchw else dxd.permute(0, 3, 1, 2).cpu()
    assert torch.equal(torch.isnan(out), torch.isnan(ref))
    m = ~torch.isnan(ref)
    assert (out[m] - ref[m]).abs().max().item() <= 1e-6 * max(1.0, ref[m].abs().max().item())  # summation order


def test_scratch_more_streams_than_table():
    """The per-(device, stream) scratch table (upr_common.h scratch(), 64
    entries): past 64 streams a single thread keeps working -- the least
    recently used entry that only this thread used is reclaimed after a device
    synchronise -- every result is right, and a reclaimed stream that comes
    back gets a fresh entry."""
    import ctypes
    import torch.nn.functional as F
    from upr import _lib as L
    torch.manual_seed(6)
    B, C, H, W = 1, 4, 16, 16
    x = torch.randn(B, C, H, W)
    xr = x.clone().requires_grad_(True)
    y = F.max_pool2d(xr, 2, 2, 0)
    gy = torch.randn(y.shape)
    y.backward(gy)
    ref = xr.grad
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    gyd = gy.permute(0, 2, 3, 1).contiguous().to(DEV)
    vx = L.UprView(xd.data_ptr(), H * W * C, W * C, C, 1)
    vg = L.UprView(gyd.data_ptr(), 8 * 8 * C, 8 * C, C, 1)
    lib = L.lib()
    # raw HIP streams (torch.cuda.Stream() hands out a pool of 32 handles)
    hip = ctypes.CDLL("libamdhip64.so")

    def run(s):
        dxd = torch.zeros(B, H, W, C, device=DEV)
        vd = L.UprView(dxd.data_ptr(), H * W * C, W * C, C, 1)
        torch.cuda.synchronize()
        rc = lib.upr_t_maxpool_bwd(ctypes.byref(vx), ctypes.byref(vg), B, H, W, C, 2, 2, 0, 8, 8,
                                   ctypes.byref(vd), s)
        assert rc == 0
        assert hip.hipStreamSynchronize(s) == 0
        assert torch.equal(dxd.permute(0, 3, 1, 2).cpu(), ref)

    live = []
    for i in range(100):  # more streams than the table holds
        s = ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(s)) == 0
        live.append(s)
        run(s)
    run(live[0])   # reclaimed meanwhile: a fresh entry
    run(live[-1])  # still in the table
    for s in live:
        assert hip.hipStreamDestroy(s) == 0


@pytest.mark.parametrize("B,C,H,W,k,s,p,acc", [
    (2, 32, 40, 56, 3, 1, 1, 1),   # EnhancedFAM branch2 (fast 3x3/1/1 path, dx accumulated)
    (2, 64, 34, 50, 2, 2, 0, 0),   # VGG pool (fast 2x2/2 path, dx written)
    (2, 64, 33, 51, 2, 2, 0, 0),   # odd extents: the uncovered last row / column get dx = 0
    (1, 6, 20, 24, 3, 1, 1, 1),    # C % 4 != 0: generic kernels
    (1, 3, 32, 32, 4, 4, 0, 0),    # generic window, written
])
def test_maxpool_code_fwd_bwd_matches_torch(B, C, H, W, k, s, p, acc):
    """upr_t_maxpool_code (forward + argmax byte codes) and upr_t_maxpool_bwd_code
    (gather from those codes) vs torch CPU max_pool2d forward / backward, NHWC,
    with ties on a 0.25 grid, one NaN window and -inf entries; the forward
    value is exact and the codes match upr_t_maxpool_bwd's recomputed ones."""
    import ctypes
    import torch.nn.functional as F
    from upr import _lib as L
    torch.manual_seed(6)
    x = (torch.randn(B, C, H, W) * 2).round() / 4
    x[0, 0, 5, 7] = float("nan")
    x[-1, -1, 2, 3] = float("-inf")
    xr = x.clone().requires_grad_(True)
    y = F.max_pool2d(xr, k, s, p)
    gy = torch.randn(y.shape)
    y.backward(gy)
    base = torch.randn(B, C, H, W)
    ref = xr.grad + (base if acc else 0)
    Ho, Wo = y.shape[2], y.shape[3]
    xd, gyd = x.permute(0, 2, 3, 1).contiguous().to(DEV), gy.permute(0, 2, 3, 1).contiguous().to(DEV)
    dxd = base.permute(0, 2, 3, 1).contiguous().to(DEV)
    yd = torch.full((B, Ho, Wo, C), 7.0, device=DEV)
    code = torch.full((B * Ho * Wo * C,), 77, dtype=torch.uint8, device=DEV)
    vx = L.UprView(xd.data_ptr(), H * W * C, W * C, C, 1)
    vy = L.UprView(yd.data_ptr(), Ho * Wo * C, Wo * C, C, 1)
    vg = L.UprView(gyd.data_ptr(), Ho * Wo * C, Wo * C, C, 1)
    vd = L.UprView(dxd.data_ptr(), H * W * C, W * C, C, 1)
    st = torch.cuda.current_stream().cuda_stream
    lib = L.lib()
    assert lib.upr_t_maxpool_code(ctypes.byref(vx), B, H, W, C, k, s, p, ctypes.byref(vy), Ho, Wo,
                                  ctypes.c_void_p(code.data_ptr()), None, st) == 0
    assert lib.upr_t_maxpool_bwd_code(ctypes.c_void_p(code.data_ptr()), ctypes.byref(vg), B, H, W, C, k, s, p, Ho, Wo,
                                      ctypes.byref(vd), acc, st) == 0
    torch.cuda.synchronize()
    yo = yd.permute(0, 3, 1, 2).cpu()
    assert torch.equal(torch.isnan(yo), torch.isnan(y.detach()))
    assert torch.equal(yo.nan_to_num(0.0), y.detach().nan_to_num(0.0))
    # the codes point at the window's first maximal tap (PyTorch's index rule)
    _, idx = F.max_pool2d(x, k, s, p, return_indices=True)
    oy = torch.arange(Ho).view(1, 1, Ho, 1) * s - p
    ox = torch.arange(Wo).view(1, 1, 1, Wo) * s - p
    want = (idx // W - oy) * k + (idx % W - ox)
    got = code.view(B, Ho, Wo, C).permute(0, 3, 1, 2).cpu().long()
    assert torch.equal(got, want)
    out = dxd.permute(0, 3, 1, 2).cpu()
    assert torch.equal(torch.isnan(out), torch.isnan(ref))
    m = ~torch.isnan(ref)
    assert (out[m] - ref[m]).abs().max().item() <= 1e-6 * max(1.0, ref[m].abs().max().item())


@pytest.mark.parametrize("B,C,H,W,k,s,p", [(2, 64, 32, 24, 2, 2, 0), (1, 32, 20, 28, 3, 1, 1), (1, 8, 33, 17, 2, 2, 0)])
def test_maxpool_bwd_code16_fuses_relu_mask(B, C, H, W, k, s, p):
    """upr_t_maxpool_bwd_code16 (the VGG pool backward with the producing
    ReLU's mask and the fp16 operand fused) equals upr_t_maxpool_bwd_code then
    upr_t_relu_mask16h bit for bit; without y16 it is the plain gather in fp16."""
    import ctypes
    from upr import _lib as L
    torch.manual_seed(9)
    x = torch.relu(torch.randn(B, H, W, C, device=DEV)).half()  # a ReLU's fp16 output (zeros included)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    y = torch.empty(B, Ho, Wo, C, device=DEV)
    code = torch.empty(B * Ho * Wo * C, dtype=torch.uint8, device=DEV)
    gy = torch.randn(B, Ho, Wo, C, device=DEV)
    vy = L.UprView(y.data_ptr(), Ho * Wo * C, Wo * C, C, 1)
    vg = L.UprView(gy.data_ptr(), Ho * Wo * C, Wo * C, C, 1)
    st = torch.cuda.current_stream().cuda_stream
    lib = L.lib()
    cp = ctypes.c_void_p(code.data_ptr())
    assert lib.upr_t_maxpool16_code(ctypes.c_void_p(x.data_ptr()), B, H, W, C, k, s, p, ctypes.byref(vy), Ho, Wo, cp,
                                    None, st) == 0
    dx = torch.empty(B, H, W, C, device=DEV)
    vd = L.UprView(dx.data_ptr(), H * W * C, W * C, C, 1)
    assert lib.upr_t_maxpool_bwd_code(cp, ctypes.byref(vg), B, H, W, C, k, s, p, Ho, Wo, ctypes.byref(vd), 0, st) == 0
    plain16 = dx.half()
    ref16 = torch.empty(B * H * W * C, dtype=torch.float16, device=DEV)
    assert lib.upr_t_relu_mask16h(ctypes.c_void_p(dx.data_ptr()), C, 0, ctypes.c_void_p(x.data_ptr()), C, B * H * W,
                                  C, ctypes.c_void_p(ref16.data_ptr()), 0, st) == 0
    got = torch.full_like(ref16, 7.0)
    assert lib.upr_t_maxpool_bwd_code16(cp, ctypes.byref(vg), B, H, W, C, k, s, p, Ho, Wo,
                                        ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(got.data_ptr()), st) == 0
    got2 = torch.full_like(ref16, 7.0)
    assert lib.upr_t_maxpool_bwd_code16(cp, ctypes.byref(vg), B, H, W, C, k, s, p, Ho, Wo, None,
                                        ctypes.c_void_p(got2.data_ptr()), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(got, ref16)
    assert torch.equal(got2, plain16.reshape(-1))
    assert (ref16 == 0).float().mean().item() > 0.3  # the mask did something


@pytest.mark.parametrize("B,C,H,W,Ho,Wo,sliced", [
    (2, 32, 16, 12, 64, 48, True),   # scale3 -> full resolution (4x) into a channel slice of the concat (vec4 path)
    (2, 32, 24, 20, 48, 40, False),  # scale2 -> full resolution (2x)
    (2, 3, 64, 48, 32, 24, False),   # the input pyramid's 0.5x downsample (generic path, C = 3)
    (1, 8, 10, 14, 37, 23, True),    # non-integer ratios
])
def test_bilinear_and_copy_vs_torch(B, C, H, W, Ho, Wo, sliced):
    """upr_t_bilinear / upr_t_bilinear_bwd (accumulating into dx) / upr_t_copy
    vs F.interpolate(mode='bilinear', align_corners=False) (models/model.py:
    436-441) forward and backward on torch CPU fp32."""
    import ctypes
    import torch.nn.functional as F
    from upr import _lib as L
    gen = torch.Generator().manual_seed(H * W + C)
    x = torch.randn(B, C, H, W, generator=gen)
    gy = torch.randn(B, C, Ho, Wo, generator=gen)
    base = torch.randn(B, C, H, W, generator=gen)
    xr = x.clone().requires_grad_(True)
    y = F.interpolate(xr, size=(Ho, Wo), mode="bilinear", align_corners=False)
    y.backward(gy)
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    CT = 3 * C if sliced else C  # the output lives in channels [C, 2C) of a wider tensor when sliced
    off = C if sliced else 0
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    yd = torch.full((B, Ho, Wo, CT), 5.0, device=DEV)
    pre = torch.randn(B, Ho, Wo, C, generator=gen).to(DEV)
    yd[..., off:off + C] = pre
    vx = L.UprView(xd.data_ptr(), H * W * C, W * C, C, 1)
    vy = L.UprView(yd.data_ptr() + 4 * off, Ho * Wo * CT, Wo * CT, CT, 1)
    assert lib.upr_t_bilinear(ctypes.byref(vx), B, H, W, C, ctypes.byref(vy), Ho, Wo, 1, st) == 0  # accumulate
    torch.cuda.synchronize()
    ref = y.detach().permute(0, 2, 3, 1) + pre.cpu()
    assert (yd[..., off:off + C].cpu() - ref).abs().max().item() <= 1e-5
    if sliced:
        assert torch.all(yd[..., :off] == 5.0) and torch.all(yd[..., off + C:] == 5.0)
    # backward from a sliced gradient, accumulated into base
    gd = torch.zeros(B, Ho, Wo, CT, device=DEV)
    gd[..., off:off + C] = gy.permute(0, 2, 3, 1).to(DEV)
    vg = L.UprView(gd.data_ptr() + 4 * off, Ho * Wo * CT, Wo * CT, CT, 1)
    dxd = base.permute(0, 2, 3, 1).contiguous().to(DEV)
    vd = L.UprView(dxd.data_ptr(), H * W * C, W * C, C, 1)
    assert lib.upr_t_bilinear_bwd(ctypes.byref(vg), B, H, W, C, Ho, Wo, ctypes.byref(vd), st) == 0
    torch.cuda.synchronize()
    refg = (xr.grad + base).permute(0, 2, 3, 1)
    assert (dxd.cpu() - refg).abs().max().item() <= 1e-5 * max(1.0, refg.abs().max().item())
    # copy (overwrite, then accumulate) between a slice and a dense tensor
    dst = torch.zeros(B, Ho, Wo, C, device=DEV)
    vdst = L.UprView(dst.data_ptr(), Ho * Wo * C, Wo * C, C, 1)
    assert lib.upr_t_copy(ctypes.byref(vy), ctypes.byref(vdst), B, Ho, Wo, C, 0, st) == 0
    assert lib.upr_t_copy(ctypes.byref(vy), ctypes.byref(vdst), B, Ho, Wo, C, 1, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst, 2 * yd[..., off:off + C])


@pytest.mark.parametrize("B,H,W,cout,acc", [(2, 40, 72, 64, 0), (1, 17, 130, 64, 1), (2, 24, 64, 32, 1)])
def test_conv_dgrad_c3_16_vs_fp64(B, H, W, cout, acc):
    """upr_t_conv_dgrad_c3_16 (VGG conv1_1's input gradient under autocast):
    vs the fp64 input gradient of the fp16-rounded dy and weights; ragged tile
    edges (H % 4, W % 64), dx accumulated or written."""
    import ctypes
    from upr import _lib as L
    gen = torch.Generator().manual_seed(H + W)
    w = torch.randn(cout, 3, 3, 3, generator=gen) * 0.2
    dy = torch.randn(B, cout, H, W, generator=gen)
    base = torch.randn(B, 3, H, W, generator=gen)
    ref = torch.nn.grad.conv2d_input((B, 3, H, W), w.half().double(), dy.half().double(), padding=1).float()
    if acc:
        ref = ref + base
    dy16 = dy.permute(0, 2, 3, 1).contiguous().half().to(DEV)
    dx = base.permute(0, 2, 3, 1).contiguous().to(DEV)
    wd = w.to(DEV)
    vd = L.UprView(dx.data_ptr(), H * W * 3, W * 3, 3, 1)
    rc = L.lib().upr_t_conv_dgrad_c3_16(ctypes.c_void_p(dy16.data_ptr()), B, H, W, ctypes.c_void_p(wd.data_ptr()),
                                        cout, ctypes.byref(vd), acc, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    _close(dx.permute(0, 3, 1, 2), ref, 1e-5, "dgrad_c3_16")


@pytest.mark.parametrize("cin,cout,H,W,skip32", [(64, 64, 32, 64, 0), (128, 64, 16, 64, 1), (256, 128, 16, 32, 1)])
def test_conv_mfma16_relu_bwd_vs_fp64(cin, cout, H, W, skip32):
    """upr_t_conv_mfma16_relu_bwd: the stride-1 input gradient of a 3x3 conv
    (the VGG shapes) with the ReLU backward of the activation it flows into
    fused into the epilogue, vs the fp64 input gradient of the fp16 dy and
    weights masked by (a > 0); fp16 copy == (half) of the fp32 output;
    skip32 leaves the fp32 buffer untouched."""
    import ctypes
    from upr import _lib as L
    gen = torch.Generator().manual_seed(cin + H)
    B = 2
    w = torch.randn(cout, cin, 3, 3, generator=gen) * 0.05
    dy = torch.randn(B, cout, H, W, generator=gen)
    a = torch.randn(B, cin, H, W, generator=gen).clamp_min(0)  # a ReLU output: about half zeros
    ref = torch.nn.grad.conv2d_input((B, cin, H, W), w.half().double(), dy.half().double(), padding=1)
    ref = (ref * (a > 0)).float().permute(0, 2, 3, 1)
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    wd = w.to(DEV)
    wt = torch.empty(w.numel(), device=DEV)
    assert lib.upr_t_pack_weight(wd.data_ptr(), wt.data_ptr(), cout, cin, 3, 3, 1, st) == 0
    wt16 = wt.half()
    dy16 = dy.permute(0, 2, 3, 1).contiguous().half().to(DEV)
    a16 = a.permute(0, 2, 3, 1).contiguous().half().to(DEV)
    y = torch.full((B, H, W, cin), 9.0, device=DEV)
    y16 = torch.empty(B * H * W * cin, dtype=torch.float16, device=DEV)
    rc = lib.upr_t_conv_mfma16_relu_bwd(dy16.data_ptr(), B, H, W, cout, wt16.data_ptr(), cin, 3, 3, 1, 1,
                                        y.data_ptr(), cin, 0, y16.data_ptr(), cin, a16.data_ptr(), cin, skip32, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    g16 = y16.view(B, H, W, cin).float()
    _close(g16, ref, 2e-3, "relu_bwd fp16")  # one fp16 rounding of the fp32 result
    assert torch.all((g16 == 0) | (a16.float() > 0))
    if skip32:
        assert torch.all(y == 9.0)
    else:
        _close(y, ref, 1e-3, "relu_bwd fp32")
        assert torch.equal(y.half().float(), g16)


@pytest.mark.parametrize("cin,cout,bias,relu,resid", [
    (96, 32, True, False, False),   # multi-scale head fusion forward (model.py:413)
    (128, 32, True, True, False),   # EnhancedFAM fusion + ReLU (model.py:49, :86)
    (32, 96, False, False, True),   # the fusion's input gradient, accumulated
    (32, 128, False, False, False),
    (64, 64, True, False, True),
])
def test_conv_mfma16_1x1_streaming(cin, cout, bias, relu, resid):
    """upr_t_conv_mfma16 on 1x1 convs with K, N <= 128 (the streaming 1x1
    kernel, conv_pw.hip): fp16 operands, fp32 output = (half)(x W^T + b) (+ the
    accumulated fp32 gradient), the fp16 copy == (half) of it; vs fp64 on the
    fp16-rounded operands."""
    from upr import _lib as L
    gen = torch.Generator().manual_seed(cin * 7 + cout)
    B, H, W = 2, 48, 64
    x = torch.randn(B, H, W, cin, generator=gen)
    w = torch.randn(cout, cin, generator=gen) * 0.1
    b = torch.randn(cout, generator=gen) if bias else None
    r = torch.randn(B, H, W, cout, generator=gen) if resid else None
    ref = x.half().double() @ w.half().double().t()
    if bias:
        ref = ref + b.double()
    if relu:
        ref = ref.clamp_min(0)
    ref = ref.float().half().float()
    if resid:
        ref = ref + r
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    xd, wd16 = x.to(DEV), w.half().to(DEV).contiguous()
    x16 = torch.empty(B * H * W * cin, dtype=torch.float16, device=DEV)
    y = r.to(DEV) if resid else torch.full((B, H, W, cout), 5.0, device=DEV)
    y16 = torch.empty(B * H * W * cout, dtype=torch.float16, device=DEV)
    bd = b.to(DEV) if bias else None
    rc = lib.upr_t_conv_mfma16(xd.data_ptr(), B, H, W, cin, cin, 0, wd16.data_ptr(), bd.data_ptr() if bias else None,
                               cout, 1, 1, 1, 0, 1, y.data_ptr() if resid else None, cout if resid else 0, int(relu),
                               y.data_ptr(), cout, 0, 0 if resid else L.UPR_T_STORE_KEEP16, x16.data_ptr(), 0,
                               y16.data_ptr(), 0, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    _close(y, ref, 1e-3, "1x1 fp32 out")
    if not resid:
        assert torch.equal(y.half().float().view(-1), y16.float())


@pytest.mark.parametrize("dil,H,W", [(1, 48, 64), (1, 20, 40), (2, 48, 64)])
def test_conv_mfma16_3x3_accumulated(dil, H, W):
    """upr_t_conv_mfma16 on a 32 -> 32 3x3 conv whose fp32 output accumulates
    into an existing gradient (res == y: the EnhancedFAM branch input
    gradients, model.py:23-51): dilation 1 on the row ring's fp32 program with
    the res32 epilogue (round 6; the generic halo kernel before), dilation 2 on
    the halo kernel; vs fp64 on the fp16-rounded operands, (half)(conv) + res."""
    import torch.nn.functional as F
    from upr import _lib as L
    gen = torch.Generator().manual_seed(dil * 100 + H)
    B, C = 2, 32
    x = torch.randn(B, C, H, W, generator=gen)
    w = torch.randn(C, C, 3, 3, generator=gen) * 0.05
    r = torch.randn(B, C, H, W, generator=gen)
    ref = F.conv2d(x.half().double(), w.half().double(), padding=dil, dilation=dil)
    ref = (ref.float().half().float() + r).permute(0, 2, 3, 1)
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    wd = w.to(DEV)
    wt = torch.empty(w.numel(), device=DEV)
    assert lib.upr_t_pack_weight(wd.data_ptr(), wt.data_ptr(), C, C, 3, 3, 0, st) == 0  # [Co][(ky, kx, ci)]
    wt16 = wt.half()
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    y = r.permute(0, 2, 3, 1).contiguous().to(DEV)
    x16 = torch.empty(B * H * W * C, dtype=torch.float16, device=DEV)
    y16 = torch.empty(B * H * W * C, dtype=torch.float16, device=DEV)
    rc = lib.upr_t_conv_mfma16(xd.data_ptr(), B, H, W, C, C, 0, wt16.data_ptr(), None, C, 3, 3, 1, dil, dil,
                               y.data_ptr(), C, 0, y.data_ptr(), C, 0, 0, x16.data_ptr(), 0, y16.data_ptr(), 0, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    _close(y, ref, 1e-3, "3x3 accumulated fp32 out")


@pytest.mark.parametrize("cin,cout", [(32, 64), (64, 128)])
def test_dgrad_1x1_stride2_scatter(cin, cout):
    """The projecting shortcut's input gradient (1x1 stride 2, model.py:119-122)
    without the zero-upsampled operand (upr_t_conv_mfma16 store | 8): dx at the
    even pixels += W^T dy, the odd pixels untouched; vs torch's conv2d_input on
    the fp16-rounded operands."""
    from upr import _lib as L
    gen = torch.Generator().manual_seed(cin + 3 * cout)
    B, Ho, Wo = 2, 32, 48
    w = torch.randn(cout, cin, 1, 1, generator=gen) * 0.1
    dy = torch.randn(B, cout, Ho, Wo, generator=gen)
    base = torch.randn(B, 2 * Ho, 2 * Wo, cin, generator=gen)
    g = torch.nn.grad.conv2d_input((B, cin, 2 * Ho, 2 * Wo), w.half().double(), dy.half().double(), stride=2)
    ref = base + g.float().half().float().permute(0, 2, 3, 1)
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    wd = w.to(DEV)
    wt = torch.empty(w.numel(), device=DEV)
    assert lib.upr_t_pack_weight(wd.data_ptr(), wt.data_ptr(), cout, cin, 1, 1, 1, st) == 0
    wt16 = wt.half()
    dyd = dy.permute(0, 2, 3, 1).contiguous().to(DEV)
    x16 = torch.empty(B * Ho * Wo * cout, dtype=torch.float16, device=DEV)
    y16 = torch.empty(16, dtype=torch.float16, device=DEV)
    gx = base.to(DEV)
    rc = lib.upr_t_conv_mfma16(dyd.data_ptr(), B, Ho, Wo, cout, cout, 0, wt16.data_ptr(), None, cin, 1, 1, 1, 0, 1,
                               gx.data_ptr(), cin, 0, gx.data_ptr(), cin, 0, L.UPR_T_STORE_S2_1X1, x16.data_ptr(), 0,
                               y16.data_ptr(), 0, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    _close(gx, ref, 1e-3, "1x1 s2 dgrad")
    odd = torch.ones(2 * Ho, 2 * Wo, dtype=torch.bool)
    odd[::2, ::2] = False
    assert torch.equal(gx.cpu()[:, odd], base[:, odd])
    # the flag is refused on anything but a 1x1 accumulate
    assert lib.upr_t_conv_mfma16(dyd.data_ptr(), B, Ho, Wo, cout, cout, 0, wt16.data_ptr(), None, cin, 1, 1, 1, 0, 1,
                                 None, 0, 0, gx.data_ptr(), cin, 0, L.UPR_T_STORE_S2_1X1, x16.data_ptr(), 0,
                                 y16.data_ptr(), 0, st) != 0


@pytest.mark.parametrize("cin,cout", [(32, 64), (64, 128), (128, 256)])
@pytest.mark.parametrize("acc,keep16", [(False, False), (True, False), (False, True)])
def test_dgrad_3x3_stride2_phases(acc, keep16, cin, cout):
    """The encoders' stride-2 input gradients (3x3 stride 2 pad 1; enc1 / enc2 /
    enc3.conv1: 32 -> 64, 64 -> 128, 128 -> 256, model.py:100-178) from dy itself
    (upr_t_conv_mfma16 store | 16: the four output phases as small convs, no
    zero-upsampled operand; register filter for the first, LDS filter slices
    for the others) vs torch's conv2d_input on the fp16-rounded operands:
    overwrite, accumulate into an existing gradient, and the fp16-only form
    (store | 2 | 4: y16 = (half) dx, dx itself not written)."""
    from upr import _lib as L
    gen = torch.Generator().manual_seed(11 + int(acc) + 2 * int(keep16) + cin)
    B, Ho, Wo = 2, 16, 48
    w = torch.randn(cout, cin, 3, 3, generator=gen) * 0.1
    dy = torch.randn(B, cout, Ho, Wo, generator=gen)
    base = torch.randn(B, 2 * Ho, 2 * Wo, cin, generator=gen)
    g = torch.nn.grad.conv2d_input((B, cin, 2 * Ho, 2 * Wo), w.half().double(), dy.half().double(), stride=2,
                                   padding=1)
    g = g.float().half().float().permute(0, 2, 3, 1)
    ref = base + g if acc else g
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    wt = torch.empty(w.numel(), device=DEV)
    assert lib.upr_t_pack_weight(w.to(DEV).data_ptr(), wt.data_ptr(), cout, cin, 3, 3, 1, st) == 0
    wt16 = wt.half()
    dyd = dy.permute(0, 2, 3, 1).contiguous().to(DEV)
    x16 = torch.empty(B * Ho * Wo * cout, dtype=torch.float16, device=DEV)
    y16 = torch.zeros(B * 4 * Ho * Wo * cin, dtype=torch.float16, device=DEV)
    gx = base.to(DEV) if acc else torch.full((B, 2 * Ho, 2 * Wo, cin), 7.0, device=DEV)
    store = L.UPR_T_STORE_S2_3X3_DGRAD | (L.UPR_T_STORE_KEEP16 | L.UPR_T_STORE_ONLY16 if keep16 else 0)
    rc = lib.upr_t_conv_mfma16(dyd.data_ptr(), B, Ho, Wo, cout, cout, 0, wt16.data_ptr(), None, cin, 3, 3, 1, 1, 1,
                               gx.data_ptr() if acc else None, cin if acc else 0, 0, gx.data_ptr(), cin, 0, store,
                               x16.data_ptr(), 0, y16.data_ptr(), 0, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    if keep16:
        _close(y16.float().view(B, 2 * Ho, 2 * Wo, cin), ref, 2e-3, "3x3 s2 dgrad (fp16 copy)")
        assert bool((gx == 7.0).all()), "only16: the fp32 output must not be written"
    else:
        _close(gx, ref, 1e-3, "3x3 s2 dgrad")


def test_shared_concat_fp16_slices():
    """A channel slice of a concat gradient's shared fp16 copy, read in place
    (EnhancedFAM's four branch convs): upr_t_conv_mfma16 store | 32 (x16 in x's
    layout), upr_t_conv_wgrad_into's dy16 in dy's layout, upr_t_chan_sum16s --
    each bit-identical to the same call on a compact copy of the slice."""
    from upr import _lib as L
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    gen = torch.Generator().manual_seed(41)
    B, H, W, C, N, k0 = 2, 16, 64, 32, 32, 64     # slice = channels 64..95 of a 128-channel concat
    cat = torch.randn(B, H, W, 4 * C, generator=gen).to(DEV)
    cat16 = cat.half()
    sl16 = cat16[..., k0:k0 + C].contiguous()
    w = (torch.randn(N, C, 3, 3, generator=gen) * 0.1).to(DEV)
    wt = torch.empty(w.numel(), device=DEV)
    assert lib.upr_t_pack_weight(w.data_ptr(), wt.data_ptr(), N, C, 3, 3, 0, st) == 0
    wt16 = wt.half()
    outs = []
    for strided in (False, True):
        y = torch.empty(B, H, W, N, device=DEV)
        y16 = torch.empty(B * H * W * N, dtype=torch.float16, device=DEV)
        if strided:
            rc = lib.upr_t_conv_mfma16(None, B, H, W, C, 4 * C, k0, wt16.data_ptr(), None, N, 3, 3, 1, 1, 1, None, 0,
                                       0, y.data_ptr(), N, 0, L.UPR_T_STORE_X16_STRIDED,
                                       ctypes.c_void_p(cat16.data_ptr() + 2 * k0), 1, y16.data_ptr(), 0, st)
        else:
            rc = lib.upr_t_conv_mfma16(None, B, H, W, C, C, 0, wt16.data_ptr(), None, N, 3, 3, 1, 1, 1, None, 0, 0,
                                       y.data_ptr(), N, 0, 0, sl16.data_ptr(), 1, y16.data_ptr(), 0, st)
        assert rc == 0, rc
        outs.append(y)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    # the ReLU-masked input-gradient form (upr_t_conv_mfma16_relu_bwd_cs) on the slice in place
    mask16 = torch.randn(B, H, W, N, generator=gen).half().to(DEV)
    mo = []
    for strided in (False, True):
        y = torch.empty(B, H, W, N, device=DEV)
        y16 = torch.empty(B * H * W * N, dtype=torch.float16, device=DEV)
        src, cs = (ctypes.c_void_p(cat16.data_ptr() + 2 * k0), 4 * C) if strided else (sl16.data_ptr(), C)
        rc = lib.upr_t_conv_mfma16_relu_bwd_cs(src, cs, B, H, W, C, wt16.data_ptr(), N, 3, 3, 1, 1, y.data_ptr(), N,
                                               0, y16.data_ptr(), N, mask16.data_ptr(), N, 0, st)
        assert rc == 0, rc
        mo.append((y, y16))
    torch.cuda.synchronize()
    assert torch.equal(mo[0][0], mo[1][0]) and torch.equal(mo[0][1], mo[1][1])
    assert torch.equal(mo[0][0] == 0, (mask16 <= 0) | (outs[0] == 0))  # zero exactly where masked
    # weight gradient: dy = the slice (fp32 strided + its fp16 copy in the same layout)
    x16 = torch.randn(B, H, W, C, generator=gen).half().to(DEV)
    dws = []
    for strided in (False, True):
        dw = torch.zeros(N, C, 3, 3, device=DEV)
        if strided:
            rc = lib.upr_t_conv_wgrad_into(None, x16.data_ptr(), B, H, W, C, C, 0, cat.data_ptr(), cat16.data_ptr(), H,
                                           W, C, 4 * C, k0, 3, 3, 1, 1, 1, dw.data_ptr(), st)
        else:
            dyc = cat[..., k0:k0 + C].contiguous()
            rc = lib.upr_t_conv_wgrad_into(None, x16.data_ptr(), B, H, W, C, C, 0, dyc.data_ptr(), sl16.data_ptr(), H,
                                           W, C, C, 0, 3, 3, 1, 1, 1, dw.data_ptr(), st)
        assert rc == 0, rc
        dws.append(dw)
    torch.cuda.synchronize()
    assert torch.equal(dws[0], dws[1])
    # channel sums of the slice's fp16 values
    ws = torch.empty((lib.upr_t_reduce_acc_doubles(C),), dtype=torch.float64, device=DEV)
    out = torch.zeros(C, device=DEV)
    assert lib.upr_t_chan_sum16s(ctypes.c_void_p(cat16.data_ptr() + 2 * k0), B * H * W, C, 4 * C, out.data_ptr(), 0,
                                 ws.data_ptr(), st) == 0
    torch.cuda.synchronize()
    ref = sl16.double().reshape(-1, C).sum(0).float().cpu()
    assert torch.allclose(out.cpu(), ref, rtol=1e-5, atol=1e-4)


def test_fp16_copy_producers():
    """The autocast operand copies written by their producers (no cast pass):
    upr_t_conv_direct16 (3 -> 32 / 64 3x3 + ReLU), upr_t_maxpool_code(y16),
    upr_t_add16, upr_t_copy16 / upr_t_bilinear16 into a channel slice of an fp16
    concat: each fp16 value == (half) of the fp32 result written alongside."""
    import ctypes
    from upr import _lib as L
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    gen = torch.Generator().manual_seed(9)
    B, H, W = 2, 20, 36
    # direct 3 -> 64 conv
    x = torch.rand(B, 3, H, W, generator=gen).to(DEV)
    w = (torch.randn(64, 3, 3, 3, generator=gen) * 0.3).to(DEV)
    bias = torch.randn(64, generator=gen).to(DEV)
    y = torch.empty(B, H, W, 64, device=DEV)
    y16 = torch.empty(B * H * W * 64, dtype=torch.float16, device=DEV)
    vx = L.UprView(x.data_ptr(), 3 * H * W, W, 1, H * W)
    vy = L.UprView(y.data_ptr(), H * W * 64, W * 64, 64, 1)
    assert lib.upr_t_conv_direct16(ctypes.byref(vx), B, H, W, 3, w.data_ptr(), bias.data_ptr(), 64, 3, 3, 1, 1, 1,
                                   ctypes.byref(vy), H, W, 1, 0, y16.data_ptr(), 0, st) == 0
    torch.cuda.synchronize()
    ref = torch.relu(torch.nn.functional.conv2d(x.cpu(), w.cpu(), bias.cpu(), padding=1)).permute(0, 2, 3, 1)
    _close(y, ref, 1e-5, "direct16 fp32")
    assert torch.equal(y16.view(B, H, W, 64), y.half())
    # skip32: the fp16 copy alone (the frozen VGG conv1_1 under autocast)
    yk = torch.full_like(y, 4.0)
    y16k = torch.empty_like(y16)
    vyk = L.UprView(yk.data_ptr(), H * W * 64, W * 64, 64, 1)
    assert lib.upr_t_conv_direct16(ctypes.byref(vx), B, H, W, 3, w.data_ptr(), bias.data_ptr(), 64, 3, 3, 1, 1, 1,
                                   ctypes.byref(vyk), H, W, 1, 0, y16k.data_ptr(), 1, st) == 0
    torch.cuda.synchronize()
    assert torch.all(yk == 4.0) and torch.equal(y16k, y16)
    # a 1 x 1 head has no fp16 form: UNSUPPORTED, nothing written
    w1 = torch.randn(1, 3, 1, 1, device=DEV)
    y1 = torch.full((B, H, W, 1), 3.0, device=DEV)
    vy1 = L.UprView(y1.data_ptr(), H * W, W, 1, 1)
    assert lib.upr_t_conv_direct16(ctypes.byref(vx), B, H, W, 3, w1.data_ptr(), None, 1, 1, 1, 1, 0, 1,
                                   ctypes.byref(vy1), H, W, 0, 0, y16.data_ptr(), 0, st) == L.UPR_ERR_UNSUPPORTED
    assert torch.all(y1 == 3.0)
    # max-pool 3x3/1/1 with the fp16 copy
    mp = torch.empty_like(y)
    mp16 = torch.empty_like(y16)
    vmp = L.UprView(mp.data_ptr(), H * W * 64, W * 64, 64, 1)
    assert lib.upr_t_maxpool_code(ctypes.byref(vy), B, H, W, 64, 3, 1, 1, ctypes.byref(vmp), H, W, None,
                                  mp16.data_ptr(), st) == 0
    torch.cuda.synchronize()
    refp = torch.nn.functional.max_pool2d(y.permute(0, 3, 1, 2).cpu(), 3, 1, 1).permute(0, 2, 3, 1)
    assert torch.equal(mp.cpu(), refp) and torch.equal(mp16.view(B, H, W, 64), mp.half())
    # the same pool from the fp16 copy (upr_t_maxpool16_code) with argmax codes
    mpa = torch.empty_like(y)
    codes = [torch.empty(B * H * W * 64, dtype=torch.uint8, device=DEV) for _ in range(2)]
    vmpa = L.UprView(mpa.data_ptr(), H * W * 64, W * 64, 64, 1)
    yh = y.half()
    assert lib.upr_t_maxpool16_code(yh.data_ptr(), B, H, W, 64, 3, 1, 1, ctypes.byref(vmpa), H, W,
                                    codes[0].data_ptr(), None, st) == 0
    assert lib.upr_t_maxpool_code(ctypes.byref(vy), B, H, W, 64, 3, 1, 1, ctypes.byref(vmp), H, W,
                                  codes[1].data_ptr(), None, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(mpa, torch.nn.functional.max_pool2d(yh.float().permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1))
    # codes: PyTorch's first-max index rule on the fp16 values
    _, idx = torch.nn.functional.max_pool2d(yh.float().permute(0, 3, 1, 2).cpu(), 3, 1, 1, return_indices=True)
    oy = torch.arange(H).view(1, 1, H, 1) - 1
    ox = torch.arange(W).view(1, 1, 1, W) - 1
    want = ((idx // W - oy) * 3 + (idx % W - ox)).permute(0, 2, 3, 1)
    assert torch.equal(codes[0].view(B, H, W, 64).cpu().long(), want)
    # ReLU mask from the fp16 copy (upr_t_relu_mask16h) == from fp32 where fp16 is exact
    g = torch.randn(B, H, W, 64, generator=gen).to(DEV)
    g16a = torch.empty(B * H * W * 64, dtype=torch.float16, device=DEV)
    yr = (y - 0.5).half()
    assert lib.upr_t_relu_mask16h(g.data_ptr(), 64, 0, yr.data_ptr(), 64, B * H * W, 64, g16a.data_ptr(), 0, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(g16a.view(B, H, W, 64), (g * (yr.float() > 0)).half())
    # add16
    s_ = torch.empty_like(y)
    s16 = torch.empty_like(y16)
    assert lib.upr_t_add16(y.data_ptr(), mp.data_ptr(), s_.data_ptr(), y.numel(), s16.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(s_, y + mp) and torch.equal(s16.view(B, H, W, 64), s_.half())
    # copy16 / bilinear16 into channels [32, 64) and [64, 96) of a 96-channel concat
    cat = torch.zeros(B, H, W, 96, device=DEV)
    cat16 = torch.zeros(B * H * W * 96, dtype=torch.float16, device=DEV)
    src = y[..., :32].contiguous()
    vs = L.UprView(src.data_ptr(), H * W * 32, W * 32, 32, 1)
    vc1 = L.UprView(cat.data_ptr() + 4 * 32, H * W * 96, W * 96, 96, 1)
    assert lib.upr_t_copy16(ctypes.byref(vs), ctypes.byref(vc1), B, H, W, 32, 0, cat16.data_ptr() + 2 * 32, 96,
                            st) == 0
    small = torch.randn(B, H // 4, W // 4, 32, generator=gen).to(DEV)
    vsm = L.UprView(small.data_ptr(), (H // 4) * (W // 4) * 32, (W // 4) * 32, 32, 1)
    vc2 = L.UprView(cat.data_ptr() + 4 * 64, H * W * 96, W * 96, 96, 1)
    assert lib.upr_t_bilinear16(ctypes.byref(vsm), B, H // 4, W // 4, 32, ctypes.byref(vc2), H, W, 0,
                                cat16.data_ptr() + 2 * 64, 96, st) == 0
    torch.cuda.synchronize()
    c16 = cat16.view(B, H, W, 96)
    assert torch.equal(cat[..., 32:64], src) and torch.equal(c16[..., 32:96], cat[..., 32:96].half())
    assert torch.all(c16[..., :32] == 0) and torch.all(cat[..., :32] == 0)
    refb = torch.nn.functional.interpolate(small.permute(0, 3, 1, 2).cpu(), size=(H, W), mode="bilinear",
                                           align_corners=False).permute(0, 2, 3, 1)
    _close(cat[..., 64:96], refb, 1e-5, "bilinear16")


@pytest.mark.parametrize("cin,cout,hw", [
    (64, 32, 12),    # width not a multiple of 16: the tile GEMM
    (64, 32, 32),    # dec1.up shape class: the streaming ConvT kernel (conv_t2.hip)
    (128, 64, 16),   # dec2.up shape class: streaming, 2 waves per pixel group
])
def test_convT_layer(cin, cout, hw):
    """fp32 ConvTranspose2d(2, 2) forward / dgrad / wgrad vs torch CPU."""
    from upr.train import Act, ConvT
    torch.manual_seed(1)
    m = torch.nn.ConvTranspose2d(cin, cout, 2, 2)
    x = torch.randn(2, cin, hw, hw)
    xr = x.clone().requires_grad_(True)
    y = m(xr)
    gy = torch.randn(y.shape)
    y.backward(gy)
    md = torch.nn.ConvTranspose2d(cin, cout, 2, 2).to(DEV)
    md.load_state_dict(m.state_dict())
    md.weight.grad = torch.zeros_like(md.weight)
    md.bias.grad = torch.zeros_like(md.bias)
    c = ConvT(md)
    c.pack()
    xa = Act(x.permute(0, 2, 3, 1).contiguous().to(DEV))
    ya = c.fwd(xa)
    _close(ya.t.permute(0, 3, 1, 2), y, 1e-4, "fwd")
    gxa = Act.new(2, hw, hw, cin, DEV)
    c.bwd(xa, Act(gy.permute(0, 2, 3, 1).contiguous().to(DEV)), gxa)
    torch.cuda.synchronize()
    _close(gxa.t.permute(0, 3, 1, 2), xr.grad, 1e-4, "dgrad")
    _close(md.weight.grad, m.weight.grad, 1e-4, "wgrad")
    _close(md.bias.grad, m.bias.grad, 1e-4, "dbias")


def test_batchnorm_train():
    from upr.train import Act, BN, relu_mask
    torch.manual_seed(2)
    m = torch.nn.BatchNorm2d(64)
    with torch.no_grad():
        m.weight.uniform_(0.5, 1.5)
        m.bias.uniform_(-0.2, 0.2)
    md = torch.nn.BatchNorm2d(64).to(DEV)
    md.load_state_dict(m.state_dict())
    md.weight.grad = torch.zeros_like(md.weight)
    md.bias.grad = torch.zeros_like(md.bias)
    x = torch.randn(2, 64, 20, 20) * 2 + 0.5
    xr = x.clone().requires_grad_(True)
    y = torch.relu(m.train()(xr))
    gy = torch.randn(y.shape)
    y.backward(gy)
    bn = BN(md)
    xa = Act(x.permute(0, 2, 3, 1).contiguous().to(DEV))
    ya = bn.fwd(xa, relu=True)
    _close(ya.t.permute(0, 3, 1, 2), y, 1e-4, "bn fwd")
    g = Act(gy.permute(0, 2, 3, 1).contiguous().to(DEV))
    relu_mask(g, ya)
    gx = Act.new(2, 20, 20, 64, DEV)
    bn.bwd(g, gx)
    torch.cuda.synchronize()
    _close(gx.t.permute(0, 3, 1, 2), xr.grad, 1e-4, "bn dgrad")
    _close(md.weight.grad, m.weight.grad, 1e-4, "dgamma")
    _close(md.bias.grad, m.bias.grad, 1e-4, "dbeta")
    _close(md.running_mean, m.running_mean, 1e-5, "running_mean")
    _close(md.running_var, m.running_var, 1e-5, "running_var")
    assert int(md.num_batches_tracked) == 1


def test_loss_terms_and_grads(golden):
    """G6 inputs on the device vs the reference's loss values and gradients."""
    from losses.loss import TotalLoss
    g = golden("g6_losses.npz")
    low, enh, illu, refl = (torch.from_numpy(g[k]).to(DEV) for k in ("low", "enh", "illu", "refl"))
    crit = TotalLoss(use_freq_loss=True).to(DEV)
    e = enh.clone().requires_grad_(True)
    i = illu.clone().requires_grad_(True)
    r = refl.clone().requires_grad_(True)
    total, d = crit(low, e, i, r)
    for k in ("exposure", "smoothness", "color", "spatial", "decouple", "perceptual", "frequency", "total"):
        np.testing.assert_allclose(d[k], float(g["dict_" + k]), rtol=1e-4, atol=1e-8, err_msg=k)
    total.backward()
    torch.cuda.synchronize()
    for name, t in (("grad_enh", e), ("grad_illu", i), ("grad_refl", r)):
        _close(t.grad, torch.from_numpy(g[name]), 1e-4, name)


def test_loss_three_channel_illumination(golden):
    """The reference self-test (losses/loss.py:806-844): B=2, 64x64 and a
    3-channel illumination map [B,3,H,W] through EdgeAwareSmoothnessLoss,
    IlluminationReflectanceDecouplingLoss and TotalLoss on the device, vs the
    reference's own values and gradients (G6c3) and the oracle."""
    from losses.loss import EdgeAwareSmoothnessLoss, IlluminationReflectanceDecouplingLoss, TotalLoss
    g = golden("g6_losses_c3.npz")
    low, enh, illu, refl = (torch.from_numpy(g[k]).to(DEV) for k in ("low", "enh", "illu", "refl"))
    assert illu.shape[1] == 3
    i = illu.clone().requires_grad_(True)
    s = EdgeAwareSmoothnessLoss().to(DEV)(i, low)
    np.testing.assert_allclose(float(s), float(g["smoothness"]), rtol=1e-4)
    s.backward()
    torch.cuda.synchronize()
    _close(i.grad, torch.from_numpy(g["grad_illu_smooth"]), 1e-4, "smooth grad_illu")
    i = illu.clone().requires_grad_(True)
    r = refl.clone().requires_grad_(True)
    dl = IlluminationReflectanceDecouplingLoss().to(DEV)(i, r)
    np.testing.assert_allclose(float(dl), float(g["decouple"]), rtol=1e-4)
    dl.backward()
    torch.cuda.synchronize()
    _close(i.grad, torch.from_numpy(g["grad_illu_decouple"]), 1e-4, "decouple grad_illu")
    _close(r.grad, torch.from_numpy(g["grad_refl_decouple"]), 1e-4, "decouple grad_refl")
    crit = TotalLoss(use_freq_loss=True).to(DEV)
    e, i, r = (t.clone().requires_grad_(True) for t in (enh, illu, refl))
    total, d = crit(low, e, i, r)
    for k in ("exposure", "smoothness", "color", "spatial", "decouple", "perceptual", "frequency", "total"):
        np.testing.assert_allclose(d[k], float(g["dict_" + k]), rtol=1e-4, atol=1e-8, err_msg=k)
    total.backward()
    torch.cuda.synchronize()
    for name, t in (("grad_enh", e), ("grad_illu", i), ("grad_refl", r)):
        _close(t.grad, torch.from_numpy(g[name]), 1e-4, name)
    with pytest.raises(NotImplementedError):
        crit(low, enh, illu[:, :2].contiguous(), refl)


def test_loss_without_reflectance(golden):
    """TotalLoss(low, enh, illu) with reflectance=None (losses/loss.py:678-682:
    the decoupling term is 0) on the device vs the reference's own value, loss
    dict and gradients w.r.t. enh / illu (G6nr, make_golden_train.py)."""
    from losses.loss import TotalLoss
    g = golden("g6_losses_norefl.npz")
    low, enh, illu = (torch.from_numpy(g[k]).to(DEV) for k in ("low", "enh", "illu"))
    crit = TotalLoss(use_freq_loss=True).to(DEV)
    e = enh.clone().requires_grad_(True)
    i = illu.clone().requires_grad_(True)
    total, d = crit(low, e, i)
    assert d["decouple"] == 0.0
    for k in ("exposure", "smoothness", "color", "spatial", "perceptual", "frequency", "total"):
        np.testing.assert_allclose(d[k], float(g["dict_" + k]), rtol=1e-4, atol=1e-8, err_msg=k)
    total.backward()
    torch.cuda.synchronize()
    for name, t in (("grad_enh", e), ("grad_illu", i)):
        _close(t.grad, torch.from_numpy(g[name]), 1e-4, name)
    # the same criterion object with a reflectance again: the decoupling term is back
    g6 = golden("g6_losses.npz")
    low, enh, illu, refl = (torch.from_numpy(g6[k]).to(DEV) for k in ("low", "enh", "illu", "refl"))
    _, d = crit(low, enh, illu, refl)
    np.testing.assert_allclose(d["decouple"], float(g6["dict_decouple"]), rtol=1e-4)
    np.testing.assert_allclose(d["total"], float(g6["dict_total"]), rtol=1e-4)


@pytest.mark.parametrize("texture,w_smooth", [("edge_density", 1.0), ("edge_density", 2.0), ("tv", 0.5)])
def test_loss_texture_methods_vs_oracle(golden, texture, w_smooth):
    """TotalLoss(texture_method, weight_smooth) on the G6 inputs: the dynamic
    smooth weight from the edge-density complexity (oracle pinned to G6's
    tex_edge) and the total + gradients against the oracle's autograd."""
    from losses.loss import TotalLoss
    from oracle import train as otrain
    g = golden("g6_losses.npz")
    low, enh, illu, refl = (torch.from_numpy(g[k]) for k in ("low", "enh", "illu", "refl"))
    crit = TotalLoss(use_freq_loss=True, texture_method=texture, weight_smooth=w_smooth).to(DEV)
    e, i, r = (t.to(DEV).clone().requires_grad_(True) for t in (enh, illu, refl))
    total, d = crit(low.to(DEV), e, i, r)
    total.backward()
    torch.cuda.synchronize()
    tex = g["tex_edge"] if texture == "edge_density" else g["tex_tv"]
    want_w = float(np.clip(w_smooth * (1.0 - 0.8 * np.mean(tex, dtype=np.float64)), 0.1, 5.0))
    # a Sobel magnitude within rounding of the 1.5x-mean threshold may flip one
    # pixel's edge bit (device FMA order vs the CPU conv): allow two flips
    B, _, H, W = low.shape
    np.testing.assert_allclose(d["smooth_weight"], want_w, rtol=1e-6,
                               atol=(0.8 * w_smooth * 2.0 / (B * H * W) if texture == "edge_density" else 0.0))
    ce, ci, cr = (t.clone().requires_grad_(True) for t in (enh, illu, refl))
    t_ref, d_ref = otrain.total_loss(otrain.vgg19_state(VGG_SEED), low, ce, ci, cr, texture_method=texture,
                                     weight_smooth=w_smooth)
    t_ref.backward()
    np.testing.assert_allclose(d["total"], d_ref["total"], rtol=1e-4)
    for name, a, b in (("grad_enh", e, ce), ("grad_illu", i, ci), ("grad_refl", r, cr)):
        _close(a.grad, b.grad, 1e-4, name)


def test_loss_adaptive_weights_dwa():
    """adaptive_weights=True (DWA, loss.py:755-798): after epoch 1 the step's
    weights come from the last two values of every term; the total equals the
    DWA-weighted sum with the dynamic smooth weight."""
    from losses.loss import TotalLoss, dwa_weights
    torch.manual_seed(4)
    low = torch.rand(2, 3, 64, 64).to(DEV) * 0.5
    crit = TotalLoss(use_freq_loss=True, adaptive_weights=True).to(DEV)
    outs = []
    for k in range(3):
        enh = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(20 + k)).to(DEV)
        illu = torch.rand(2, 1, 64, 64, generator=torch.Generator().manual_seed(30 + k)).to(DEV) * 0.8 + 0.1
        refl = enh / (illu + 1e-6)
        with torch.no_grad():
            outs.append(crit(low, enh, illu, refl, epoch=2 if k == 2 else 1)[1])
    hist = {key: [o[key] for o in outs[:2]] for key in crit.loss_history}
    w = dwa_weights(hist, crit._weights)
    w["smoothness"] = outs[2]["smooth_weight"]
    want = sum(w[key] * outs[2][key] for key in w)
    np.testing.assert_allclose(outs[2]["total"], want, rtol=1e-5)
    assert len(crit.loss_history["exposure"]) == 3


def _model(pre, aspp, seed=0):
    from models.model import UP_Retinex
    torch.manual_seed(seed)
    return UP_Retinex(use_preact=pre, use_aspp=aspp)


def test_train_step_matches_reference_g7(golden):
    """One trainers/train.py step body (plain model, seed 0, B=2 64x64) vs the
    reference's own step recorded in G7."""
    from losses.loss import TotalLoss
    from trainers.train import make_optimizer, train_step
    g = golden("g7_train_step.npz")
    model = _model(False, False).to(DEV)
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.train()
    crit = TotalLoss(use_freq_loss=True).to(DEV)
    opt = make_optimizer(model, lr=1e-4, weight_decay=1e-5)
    x = torch.from_numpy(g["x"]).to(DEV)
    loss, d = train_step(model, x, crit, opt)
    torch.cuda.synchronize()
    for k in ("total", "exposure", "smoothness", "color", "spatial", "decouple", "perceptual", "frequency"):
        np.testing.assert_allclose(d[k], float(g["dict_" + k]), rtol=1e-4, atol=1e-9, err_msg=k)
    names = [str(n) for n in g["param_names"]]
    params = dict(model.named_parameters())
    norm = float(g["clip_norm"])
    coef = min(1.0, 1.0 / (norm + 1e-6))
    gn = np.array([float(params[n].grad.norm()) * coef for n in names])
    # conv biases feeding a BatchNorm have an exactly-zero true gradient: their
    # norms are rounding noise in both implementations, hence the absolute floor
    np.testing.assert_allclose(gn, g["grad_norm"], rtol=1e-3, atol=1e-6 * float(g["grad_norm"].max()))
    for n in names:
        key = "grad/" + n
        if key in g.files:
            _close(params[n].grad * coef, torch.from_numpy(g[key]), 2e-3, key)
    sd = model.state_dict()
    dn = np.array([float((sd[n].cpu() - sd0[n].cpu()).norm()) for n in names])
    # Adam normalises each element by sqrt(v): a noise-level gradient (the
    # BN-fed conv biases above) still moves its parameter by ~lr, so those are
    # compared against the step size rather than relatively
    noise = gn < 1e-6 * gn.max()
    np.testing.assert_allclose(dn[~noise], g["delta_norm"][~noise], rtol=1e-3, atol=1e-11)
    assert np.all(dn[noise] <= 1e-4 * np.sqrt([params[n].numel() for n in np.array(names)[noise]]) * 1.01)
    for k in g["buf_names"]:
        _close(sd[str(k)], torch.from_numpy(g["buf/" + str(k)]), 1e-4, str(k))


@pytest.mark.parametrize("pre,aspp", [(True, False), (False, True), (True, True)])
def test_train_grads_variants_vs_oracle(pre, aspp):
    """Training-mode forward + backward of the other variants vs the oracle
    (oracle/net.py train mode + oracle/train.py losses), the ASPP Dropout mask
    replayed from the device.

    Tolerance: the oracle is run in fp64 (the exact answer) and in fp32 (the
    reference's own arithmetic).  Small-batch BatchNorm makes fp32 training
    gradients noisy — the fp32 CPU oracle itself deviates from fp64 by up to
    ~2e-2 of a tensor's max on the ASPP variants (the global-pool BN normalises
    over B values) — so per tensor the device gradient's relative L2 error vs
    fp64 must be within max(4 x the fp32 oracle's, 2 x the median over all
    tensors of the fp32 oracle's, 1e-3), and its max|d| within
    max(8 x the fp32 oracle's, that median floor x max|g64|, 5e-3 x max|g64|), the fp32 oracle's
    deviation being the larger of two runs with different CPU kernels (NCHW
    and channels-last inputs: two summation orders): a different summation
    order lands anywhere in that noise band, a wrong kernel lands far outside.  B = 4:
    the ASPP global-pool BatchNorm normalises over the batch only (over B = 2
    its input gradient is exactly zero, pure rounding noise)."""
    from oracle import net as onet
    from oracle import train as otrain
    from losses.loss import TotalLoss
    B = 4
    model = _model(pre, aspp, seed=3)
    sd_cpu = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    crit = TotalLoss(use_freq_loss=True).to(DEV)
    x = torch.rand(B, 3, 64, 64, generator=torch.Generator().manual_seed(5)) * 0.6
    enh, refl, illu = model(x.to(DEV))
    total, d = crit(x.to(DEV), enh, illu, refl)
    st = model.__dict__["_upr_train"]
    total.backward()
    torch.cuda.synchronize()
    mask = None
    if aspp:
        asp = [b for b in st["graph"].ie.mid if type(b).__name__ == "ASPPT"][0]
        mask = asp.mask.cpu().view(B, 8, 8, 256).permute(0, 3, 1, 2).float()
    names = otrain.param_names(sd_cpu)
    vgg = otrain.vgg19_state(VGG_SEED)

    def oracle(dt, channels_last=False):
        s2 = {k: (v.to(dt) if v.is_floating_point() else v.clone()) for k, v in sd_cpu.items()}
        params = {k: s2[k].clone().requires_grad_(True) for k in names}
        work = dict(s2)
        work.update(params)
        xin = x.to(dt)
        if channels_last:  # same arithmetic, other CPU kernels / summation order
            xin = xin.contiguous(memory_format=torch.channels_last)
        with otrain.train_mode(dropout_mask=lambda shape: mask.to(dt)):
            e_r, r_r, i_r = onet.forward(work, xin, pre, aspp)
        t_r, d_r = otrain.total_loss({k: v.to(dt) for k, v in vgg.items()}, x.to(dt), e_r, i_r, r_r)
        t_r.backward()
        return e_r, i_r, d_r, {k: params[k].grad.double() for k in names}

    e64, i64, d64, g64 = oracle(torch.float64)
    _, _, _, g32 = oracle(torch.float32)
    _, _, _, g32b = oracle(torch.float32, channels_last=True)
    _close(enh, e64, 1e-4, "enh")
    _close(illu, i64, 1e-4, "illu")
    np.testing.assert_allclose(d["total"], d64["total"], rtol=1e-4)
    dev_params = dict(model.named_parameters())
    gmax = max(v.abs().max().item() for v in g64.values())
    rows = []
    for n in names:
        ref = g64[n]
        if ref.abs().max().item() < 1e-9 * gmax:
            continue  # BN-fed conv bias: zero true gradient (rounding noise)
        dev = dev_params[n].grad.double().cpu()
        dev_err = (dev - ref).abs().max().item()
        cpu_err = max((g32[n] - ref).abs().max().item(), (g32b[n] - ref).abs().max().item())
        rn = ref.norm().item()
        dev_l2 = (dev - ref).norm().item() / rn
        cpu_l2 = max((g32[n] - ref).norm().item(), (g32b[n] - ref).norm().item()) / rn
        rows.append((n, ref, dev_err, cpu_err, dev_l2, cpu_l2))
    # the batch-statistics amplification perturbs the whole gradient by a
    # similar relative amount, so a tensor whose own fp32 CPU deviation landed
    # low is also judged against the network-wide fp32 noise level (median)
    floor_l2 = 2.0 * float(np.median([r[5] for r in rows]))
    for n, ref, dev_err, cpu_err, dev_l2, cpu_l2 in rows:
        print(f"{n}: max|d| dev {dev_err:.3e} cpu32 {cpu_err:.3e}; rel-L2 dev {dev_l2:.3e} cpu32 {cpu_l2:.3e}")
        tol_l2 = max(4.0 * cpu_l2, floor_l2, 1e-3)
        assert dev_l2 <= tol_l2, f"grad {n}: device rel-L2 {dev_l2:.3e} vs fp64 > {tol_l2:.3e} (fp32 CPU {cpu_l2:.3e})"
        tol = max(8.0 * cpu_err, floor_l2 * ref.abs().max().item(), 5e-3 * ref.abs().max().item()) + 1e-9
        assert dev_err <= tol, f"grad {n}: device |d| {dev_err:.3e} vs fp64 > {tol:.3e} (fp32 CPU |d| {cpu_err:.3e})"


@pytest.mark.parametrize("pre", [False, True])
def test_train_grads_b8_vs_fp64(pre):
    """The no-ASPP variants at B = 8, 64x64 against the fp64 oracle, per
    parameter tensor, with the per-tensor fp32 CPU oracle as the yardstick and
    NO network-wide floor: device rel-L2 <= max(4 x the fp32 oracle's, 2e-3),
    max|d| <= max(4 x the fp32 oracle's, 2e-2 x max|g|).  Both are fp32 with
    different reduction orders; the largest rel-L2 ratio seen on MI355X is 2.4x
    (enc1.bn1.weight 5.0e-3 vs 2.3e-3, dec2.conv.0.weight 3.8e-3 vs 1.6e-3:
    the tensors deepest in the backward pass carry the most accumulated
    rounding); single elements are noisier (dec2.conv.3.weight 1.4e-2 of
    max|g| vs 1.8e-3 on the CPU, dec3.conv.3.weight 3.1e-2 vs 2.1e-2).

    Plus a FIXED bound, independent of the CPU yardstick: every tensor's
    rel-L2 <= 1e-2 (worst seen on MI355X 6.4e-3; the fp32 CPU oracle itself
    reaches 4.0e-3 here, where fp32 rounding flips a loss-term branch), and
    the median over the model's tensors <= 2e-3."""
    from oracle import net as onet
    from oracle import train as otrain
    from losses.loss import TotalLoss
    B = 8
    model = _model(pre, False, seed=4)
    sd_cpu = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    crit = TotalLoss(use_freq_loss=True).to(DEV)
    x = torch.rand(B, 3, 64, 64, generator=torch.Generator().manual_seed(6)) * 0.6
    enh, refl, illu = model(x.to(DEV))
    total, d = crit(x.to(DEV), enh, illu, refl)
    total.backward()
    torch.cuda.synchronize()
    names = otrain.param_names(sd_cpu)
    vgg = otrain.vgg19_state(VGG_SEED)

    def oracle(dt):
        s2 = {k: (v.to(dt) if v.is_floating_point() else v.clone()) for k, v in sd_cpu.items()}
        params = {k: s2[k].clone().requires_grad_(True) for k in names}
        work = dict(s2)
        work.update(params)
        with otrain.train_mode():
            e_r, r_r, i_r = onet.forward(work, x.to(dt), pre, False)
        t_r, d_r = otrain.total_loss({k: v.to(dt) for k, v in vgg.items()}, x.to(dt), e_r, i_r, r_r)
        t_r.backward()
        return d_r, {k: params[k].grad.double() for k in names}

    d64, g64 = oracle(torch.float64)
    _, g32 = oracle(torch.float32)
    np.testing.assert_allclose(d["total"], d64["total"], rtol=1e-4)
    dev_params = dict(model.named_parameters())
    gmax = max(v.abs().max().item() for v in g64.values())
    worst, l2s = (0.0, 0.0), []
    for n in names:
        ref = g64[n]
        if ref.abs().max().item() < 1e-9 * gmax:
            continue  # BN-fed conv bias: zero true gradient
        dev = dev_params[n].grad.double().cpu()
        rn, rm = ref.norm().item(), ref.abs().max().item()
        l2, l2c = (dev - ref).norm().item() / rn, (g32[n] - ref).norm().item() / rn
        mx, mxc = (dev - ref).abs().max().item(), (g32[n] - ref).abs().max().item()
        worst = max(worst, (l2, l2c))
        l2s.append(l2)
        print(f"{n}: rel-L2 dev {l2:.3e} cpu32 {l2c:.3e}; max|d| dev {mx / rm:.3e} cpu32 {mxc / rm:.3e} (of max|g|)")
        assert l2 <= max(4.0 * l2c, 2e-3), f"grad {n}: rel-L2 {l2:.3e} (fp32 CPU {l2c:.3e})"
        assert mx <= max(4.0 * mxc, 2e-2 * rm), f"grad {n}: max|d| {mx:.3e} (fp32 CPU {mxc:.3e})"
    print(f"pre={pre}: worst (device, fp32 CPU) rel-L2 vs fp64 {worst}; median device {np.median(l2s):.3e}")
    assert max(l2s) <= 1e-2 and float(np.median(l2s)) <= 2e-3


def test_train_graph_frozen_bn_and_eval_aspp_vs_oracle():
    """model.train() followed by .eval() on one BatchNorm and on the ASPP module
    (the fine-tuning pattern): those modules use their running statistics and
    no Dropout in the forward, so their backward is the affine map (dx = g *
    gamma * invstd, not the batch-statistics form) while dgamma / dbeta still
    accumulate.  Forward + backward of a random projection of the outputs vs
    the fp64 oracle with the same modules in eval mode: per tensor rel-L2 <=
    max(4 x the fp32 oracle's, 2e-3).  The batch-statistics backward on those
    modules would be off by O(1)."""
    from oracle import net as onet
    from oracle import train as otrain
    B = 4
    model = _model(True, True, seed=5)
    with torch.no_grad():  # non-trivial running statistics for the frozen modules
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)
    sd_cpu = {k: v.detach().clone() for k, v in model.state_dict().items()}
    sd0 = {k: v.clone() for k, v in sd_cpu.items()}  # the fp32 oracle run updates sd_cpu's buffers in place
    model = model.to(DEV).train()
    model.ie_net.enc2.bn1.eval()
    model.ie_net.bottleneck[1].eval()
    frozen = ("ie_net.enc2.bn1", "ie_net.bottleneck.1.")
    x = torch.rand(B, 3, 64, 64, generator=torch.Generator().manual_seed(8)) * 0.6
    gen = torch.Generator().manual_seed(9)
    r = [torch.randn(s, generator=gen) for s in ((B, 3, 64, 64), (B, 3, 64, 64), (B, 1, 64, 64))]
    outs = model(x.to(DEV))
    sum((o * ri.to(DEV)).sum() for o, ri in zip(outs, r)).backward()
    torch.cuda.synchronize()
    names = otrain.param_names(sd_cpu)

    def oracle(dt):
        s2 = {k: (v.to(dt) if v.is_floating_point() else v.clone()) for k, v in sd_cpu.items()}
        params = {k: s2[k].clone().requires_grad_(True) for k in names}
        work = dict(s2)
        work.update(params)
        with otrain.train_mode(eval_prefixes=frozen):
            o_r = onet.forward(work, x.to(dt), True, True)
        sum((o * ri.to(dt)).sum() for o, ri in zip(o_r, r)).backward()
        return o_r, {k: params[k].grad.double() for k in names}, work

    o64, g64, w64 = oracle(torch.float64)
    _, g32, _ = oracle(torch.float32)
    for o, o_r in zip(outs, o64):
        _close(o, o_r, 1e-4, "output")
    # the frozen modules' running statistics are untouched, the others moved
    for k, v in model.state_dict().items():
        if k.endswith("running_mean"):
            same = torch.equal(v.cpu(), sd0[k])
            assert same == k.startswith(frozen), k
            _close(v, w64[k], 1e-5, k)
    dev_params = dict(model.named_parameters())
    gmax = max(v.abs().max().item() for v in g64.values())
    for n in names:
        ref = g64[n]
        if ref.abs().max().item() < 1e-9 * gmax:
            continue  # BN-fed conv bias: zero true gradient
        rn = ref.norm().item()
        l2 = (dev_params[n].grad.double().cpu() - ref).norm().item() / rn
        l2c = (g32[n] - ref).norm().item() / rn
        assert l2 <= max(4.0 * l2c, 2e-3), f"grad {n}: rel-L2 {l2:.3e} (fp32 CPU {l2c:.3e})"


def _amp_setup(seed=0):
    from losses.loss import TotalLoss
    from trainers.train import make_optimizer
    model = _model(False, False, seed=seed).to(DEV).train()
    crit = TotalLoss(use_freq_loss=True).to(DEV)
    opt = make_optimizer(model, lr=1e-4, weight_decay=1e-5)
    return model, crit, opt


def test_amp_gradscaler_step_equals_fp32_step():
    """The AMP branch's control flow (train.py:71-89) with fp32 arithmetic
    (amp_fp16=False) and a power-of-two loss scale: scaling commutes exactly
    with every rounding, so after unscale_ the gradients, the clipped Adam
    update and the parameters equal the no-AMP step's."""
    from trainers.train import GradScaler, train_step
    x = (torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(11)) * 0.5).to(DEV)
    m1, c1, o1 = _amp_setup()
    train_step(m1, x, c1, o1)
    m2, c2, o2 = _amp_setup()
    scaler = GradScaler(init_scale=2.0 ** 16)
    l2, d2 = train_step(m2, x, c2, o2, scaler=scaler, use_amp=True, amp_fp16=False)
    torch.cuda.synchronize()
    assert scaler.get_scale() == 2.0 ** 16  # finite step, growth interval not reached
    p1 = dict(m1.named_parameters())
    for n, p in m2.named_parameters():
        _close(p, p1[n], 1e-6, n)


def test_amp_gradscaler_skips_nonfinite_step():
    """An inf gradient: the step is skipped (parameters and Adam state
    untouched), the scale backs off by 0.5, and the next finite step runs."""
    from trainers.train import GradScaler, clip_grad_norm_
    x = (torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(12)) * 0.5).to(DEV)
    model, crit, opt = _amp_setup(seed=1)
    scaler = GradScaler(init_scale=1024.0)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    opt.zero_grad()
    enh, refl, illu = model(x)
    loss, _ = crit(x, enh, illu, refl)
    scaler.scale(loss).backward()
    next(iter(model.parameters())).grad.view(-1)[0] = float("inf")
    scaler.unscale_(opt)
    clip_grad_norm_(model.parameters(), 1.0)
    scaler.step(opt)
    scaler.update()
    torch.cuda.synchronize()
    assert scaler.get_scale() == 512.0
    assert opt.step_count == 0
    for n, p in model.named_parameters():
        assert torch.equal(p.detach(), before[n]), n
    from trainers.train import train_step
    train_step(model, x, crit, opt, scaler=scaler, use_amp=True)
    torch.cuda.synchronize()
    assert opt.step_count == 1 and scaler.get_scale() == 512.0
    moved = sum(int(not torch.equal(p.detach(), before[n])) for n, p in model.named_parameters())
    assert moved > 0


def test_amp_autocast_fp16_gradients_vs_oracle():
    """The reference's AMP step runs forward + loss under autocast (train.py:72):
    convs in fp16.  With autocast on, the engine computes every MFMA conv (and its
    input gradient, model and VGG) with fp16 operands and fp32 accumulation.

    Oracle: oracle/net.py + oracle/train.py in fp64, plain (g64) and with the
    autocast conv arithmetic emulated (net.amp_conv: fp16-rounded operands and
    outputs, g16).  g16 - g64 is the perturbation fp16 convs cause by
    themselves; BatchNorm over a small batch amplifies it (B = 4 here).  Per
    parameter the device gradient must lie within max(2 x that band, 2 x its
    median over the model, 1e-3) of g64 (rel-L2), and the loss terms within
    rel 1e-3 of the emulation's."""
    from oracle import net as onet
    from oracle import train as otrain
    from losses.loss import TotalLoss
    B = 4
    model = _model(False, False, seed=3)
    sd_cpu = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    crit = TotalLoss(use_freq_loss=True).to(DEV)
    x = torch.rand(B, 3, 64, 64, generator=torch.Generator().manual_seed(5)) * 0.6
    with torch.autocast("cuda", dtype=torch.float16):
        enh, refl, illu = model(x.to(DEV))
        total, d = crit(x.to(DEV), enh, illu, refl)
    total.backward()
    torch.cuda.synchronize()
    g = model.__dict__["_upr_train"]["graph"]
    assert all(c.amp for c in g._convs if getattr(c, "mfma", True)), "autocast step did not use the fp16 conv path"
    names = otrain.param_names(sd_cpu)
    vgg = otrain.vgg19_state(VGG_SEED)

    def oracle(amp):
        s2 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd_cpu.items()}
        params = {k: s2[k].clone().requires_grad_(True) for k in names}
        work = dict(s2)
        work.update(params)
        with otrain.train_mode(amp=amp):
            e_r, r_r, i_r = onet.forward(work, x.double(), False, False)
            t_r, d_r = otrain.total_loss({k: v.double() for k, v in vgg.items()}, x.double(), e_r, i_r, r_r)
        t_r.backward()
        return d_r, {k: params[k].grad for k in names}

    d64, g64 = oracle(False)
    d16, g16 = oracle(True)
    for k in ("total", "exposure", "smoothness", "color", "spatial", "decouple", "perceptual", "frequency"):
        np.testing.assert_allclose(d[k], d16[k], rtol=1e-3, atol=1e-9, err_msg=k)
    dev_params = dict(model.named_parameters())
    gmax = max(v.abs().max().item() for v in g64.values())
    rows = []
    for n in names:
        ref = g64[n]
        if ref.abs().max().item() < 1e-9 * gmax:
            continue  # BN-fed conv bias: zero true gradient
        rn = ref.norm().item()
        dev = (dev_params[n].grad.double().cpu() - ref).norm().item() / rn
        band = (g16[n] - ref).norm().item() / rn
        rows.append((n, dev, band))
    floor = 2.0 * float(np.median([r[2] for r in rows]))
    for n, dev, band in rows:
        print(f"{n}: rel-L2 vs fp64 device-AMP {dev:.3e}, emulated autocast {band:.3e}")
        tol = max(2.0 * band, floor, 1e-3)
        assert dev <= tol, f"{n}: AMP gradient rel-L2 {dev:.3e} > {tol:.3e} (autocast band {band:.3e})"


@pytest.mark.parametrize("amp", [False, True])
def test_train_step_full_size_bs8_512(amp):
    """configs[4] at full size (B=8, 512x512, plain model, TotalLoss with the
    frequency term): the loss and every gradient are finite and the step moves
    the parameters.  The loss dict of the first two images (B=2 at 512x512) is
    checked against the CPU oracle's (oracle/train.py, fp32 torch autograd):
    rel 1e-4 in fp32, 1e-2 with autocast fp16 arithmetic."""
    from losses.loss import TotalLoss
    from oracle import net as onet
    from oracle import train as otrain
    from trainers.train import GradScaler, make_optimizer, train_step
    x = torch.rand(8, 3, 512, 512, generator=torch.Generator().manual_seed(2))
    # B = 2 loss dict vs the oracle
    model = _model(False, False, seed=0)
    sd_cpu = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    crit = TotalLoss(use_freq_loss=True).to(DEV)
    with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
        enh, refl, illu = model(x[:2].to(DEV))
        _, d = crit(x[:2].to(DEV), enh, illu, refl)
    torch.cuda.synchronize()
    names = otrain.param_names(sd_cpu)
    work = dict(sd_cpu)
    with otrain.train_mode():
        e_r, r_r, i_r = onet.forward(work, x[:2], False, False)
    with torch.no_grad():
        _, d_r = otrain.total_loss(otrain.vgg19_state(VGG_SEED), x[:2], e_r, i_r, r_r)
    for k in ("total", "exposure", "smoothness", "color", "spatial", "decouple", "perceptual", "frequency"):
        np.testing.assert_allclose(d[k], d_r[k], rtol=1e-2 if amp else 1e-4, atol=1e-8, err_msg=k)
    # full B = 8 step
    model = _model(False, False, seed=0).to(DEV).train()
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    opt = make_optimizer(model, lr=1e-4, weight_decay=1e-5)
    scaler = GradScaler() if amp else None
    loss, d8 = train_step(model, x.to(DEV), crit, opt, scaler=scaler, use_amp=amp)
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in d8.values()), d8
    gn = sum(float(p.grad.double().norm() ** 2) for p in model.parameters()) ** 0.5
    assert np.isfinite(gn) and gn > 0
    moved = sum(int(not torch.equal(p.detach(), before[n])) for n, p in model.named_parameters())
    assert moved > len(before) // 2
    print(f"bs8 512^2 step (amp={amp}): loss {d8['total']:.6g}, gradient norm before clipping {gn:.4g}")


_G512 = {}


def _oracle_grads_512(sd_cpu, x, amp):
    """fp64 oracle gradients of TotalLoss at B=2 512x512 (plain model); amp:
    with the autocast conv arithmetic emulated (net.amp_conv).  Cached per amp:
    one oracle pass takes ~40 s on 16 host cores."""
    from oracle import net as onet
    from oracle import train as otrain
    if amp not in _G512:
        names = otrain.param_names(sd_cpu)
        s2 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd_cpu.items()}
        params = {k: s2[k].clone().requires_grad_(True) for k in names}
        work = dict(s2)
        work.update(params)
        with otrain.train_mode(amp=amp):
            e_r, r_r, i_r = onet.forward(work, x.double(), False, False)
            t_r, d_r = otrain.total_loss({k: v.double() for k, v in otrain.vgg19_state(VGG_SEED).items()},
                                         x.double(), e_r, i_r, r_r)
        t_r.backward()
        _G512[amp] = (d_r, {k: params[k].grad for k in names})
    return _G512[amp]


@pytest.mark.parametrize("amp", [False, True])
def test_train_grads_512_b2_fixed_bound(amp):
    """configs[4]'s arithmetic at its image size (reference trainers/train.py:63-103,
    B=2 of the bs8 512x512 step, plain model, TotalLoss with the frequency term):
    every parameter gradient vs the fp64 oracle under a FIXED bound.

    fp32: per tensor rel-L2 <= 5e-3, median over the model <= 1e-3.
    autocast fp16 (train.py:72): per tensor rel-L2 <= max(2 x the emulated
    autocast band, 2 x the band's median, 5e-3), where the band is
    |g_amp_emulated - g64| / |g64| from the fp64 oracle with fp16-rounded conv
    operands and outputs (the perturbation fp16 convs cause by themselves)."""
    from losses.loss import TotalLoss
    from oracle import train as otrain
    x = torch.rand(2, 3, 512, 512, generator=torch.Generator().manual_seed(21)) * 0.6
    model = _model(False, False, seed=7)
    sd_cpu = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    crit = TotalLoss(use_freq_loss=True).to(DEV)
    with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
        enh, refl, illu = model(x.to(DEV))
        total, d = crit(x.to(DEV), enh, illu, refl)
    total.backward()
    torch.cuda.synchronize()
    if amp:
        g = model.__dict__["_upr_train"]["graph"]
        assert all(c.amp for c in g._convs if getattr(c, "mfma", True)), "autocast step did not use the fp16 convs"
    names = otrain.param_names(sd_cpu)
    d64, g64 = _oracle_grads_512(sd_cpu, x, False)
    if amp:
        d16, g16 = _oracle_grads_512(sd_cpu, x, True)
        for k in ("total", "exposure", "smoothness", "color", "spatial", "decouple", "perceptual", "frequency"):
            np.testing.assert_allclose(d[k], d16[k], rtol=1e-3, atol=1e-9, err_msg=k)
    else:
        np.testing.assert_allclose(d["total"], d64["total"], rtol=1e-4)
    dev_params = dict(model.named_parameters())
    gmax = max(v.abs().max().item() for v in g64.values())
    rows = []
    for n in names:
        ref = g64[n]
        if ref.abs().max().item() < 1e-9 * gmax:
            continue  # BN-fed conv bias: zero true gradient
        rn = ref.norm().item()
        l2 = (dev_params[n].grad.double().cpu() - ref).norm().item() / rn
        band = (g16[n] - ref).norm().item() / rn if amp else 0.0
        rows.append((n, l2, band))
    med = float(np.median([r[1] for r in rows]))
    bmed = float(np.median([r[2] for r in rows]))
    for n, l2, band in rows:
        print(f"{n}: rel-L2 vs fp64 {l2:.3e}" + (f" (emulated autocast band {band:.3e})" if amp else ""))
    print(f"512^2 B=2 amp={amp}: worst rel-L2 {max(r[1] for r in rows):.3e}, median {med:.3e}")
    for n, l2, band in rows:
        tol = max(2.0 * band, 2.0 * bmed, 5e-3) if amp else 5e-3
        assert l2 <= tol, f"{n}: rel-L2 {l2:.3e} > {tol:.3e}"
    if not amp:
        assert med <= 1e-3, med


@pytest.mark.parametrize("M,C", [(8 * 64 * 64, 32), (2 * 40 * 24, 64), (8 * 32 * 32, 256), (100, 4)])
def test_bn_stats16_fin_matches_two_step(M, C):
    """upr_t_bn_stats16_fin (slot sums + finalise in one kernel) equals
    upr_t_bn_stats16 followed by upr_t_bn_finalize bit for bit: acc, mean,
    invstd, running mean / variance and num_batches_tracked."""
    from upr import _lib as L
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    gen = torch.Generator().manual_seed(13)
    x16 = (torch.randn(M, C, generator=gen) * 2 + 0.5).half().to(DEV)
    nacc = lib.upr_t_reduce_acc_doubles(C)
    outs = []
    for fused in (False, True):
        acc = torch.zeros(nacc, dtype=torch.float64, device=DEV)
        rm = torch.linspace(-1, 1, C, device=DEV)
        rv = torch.linspace(0.5, 2, C, device=DEV)
        nbt = torch.tensor(7, dtype=torch.int64, device=DEV)
        mean, inv = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        args = (ctypes.c_float(0.1), ctypes.c_float(1e-5), rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(),
                mean.data_ptr(), inv.data_ptr())
        if fused:
            assert lib.upr_t_bn_stats16_fin(x16.data_ptr(), M, C, acc.data_ptr(), *args, st) == 0
        else:
            assert lib.upr_t_bn_stats16(x16.data_ptr(), M, C, acc.data_ptr(), st) == 0
            assert lib.upr_t_bn_finalize(acc.data_ptr(), M, C, *args, st) == 0
        torch.cuda.synchronize()
        outs.append((acc[:2 * C].clone(), mean, inv, rm, rv, nbt))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    assert int(outs[1][5]) == 8


@pytest.mark.parametrize("n", [4096, 8 * 64 * 64 * 256])
def test_mse16_matches_fp32_mse(n):
    """upr_t_mse16 (the perceptual MSE over the frozen VGG's fp16-only features
    under autocast, losses/loss.py:198-211) vs upr_t_mse on the same values
    widened to fp32 (the pooled features are exact fp16 values): the mean of
    squares within fp64 summation order, the gradient 2 * scale * d bit-exact."""
    from upr import _lib as L
    gen = torch.Generator().manual_seed(n % 97)
    a = torch.randn(n, generator=gen).half()
    b = torch.randn(n, generator=gen).half()
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    a16, b16 = a.to(DEV), b.to(DEV)
    a32, b32 = a16.float(), b16.float()
    acc = torch.zeros(2, dtype=torch.float64, device=DEV)
    g16 = torch.empty(n, device=DEV)
    g32 = torch.empty(n, device=DEV)
    scale = 0.25 / n
    assert lib.upr_t_mse16(a16.data_ptr(), b16.data_ptr(), n, acc.data_ptr(), g16.data_ptr(), ctypes.c_float(scale),
                           st) == 0
    assert lib.upr_t_mse(a32.data_ptr(), b32.data_ptr(), n, acc.data_ptr() + 8, g32.data_ptr(), ctypes.c_float(scale),
                         st) == 0
    torch.cuda.synchronize()
    ref = ((a.double() - b.double()) ** 2).mean().item()
    assert abs(acc[0].item() - ref) <= 1e-12 * max(ref, 1.0)
    assert abs(acc[0].item() - acc[1].item()) <= 1e-12 * max(ref, 1.0)
    assert torch.equal(g16, g32)
    # unsupported layouts decline instead of computing
    assert lib.upr_t_mse16(a16.data_ptr(), b16.data_ptr(), n - 1, acc.data_ptr(), None, ctypes.c_float(1.0),
                           st) == L.UPR_ERR_UNSUPPORTED


def test_amp_fp16_only_stores_bitwise():
    """The autocast step's fp16-only activation stores (upr/train.py
    FP16_ONLY_STORES: the EnhancedFAM and ASPP concats, the FAM branch / pool
    outputs, the scale stems) only skip fp32 values nothing reads: the
    parameter gradients and loss terms of a preact+ASPP step at 512^2 (every
    store form active: widths multiples of 64 at the FAM and the ASPP) are
    bit-identical with the stores on and off."""
    from losses.loss import TotalLoss
    from upr import train as T

    def step(only):
        T.FP16_ONLY_STORES[0] = only
        try:
            torch.manual_seed(11)
            model = _model(True, True, seed=3).to(DEV).train()
            crit = TotalLoss(use_freq_loss=True).to(DEV)
            x = (torch.rand(2, 3, 512, 512, generator=torch.Generator().manual_seed(6)) * 0.6).to(DEV)
            with torch.autocast("cuda", dtype=torch.float16):
                enh, refl, illu = model(x)
                total, d = crit(x, enh, illu, refl)
            total.backward()
            torch.cuda.synchronize()
            g = model.__dict__["_upr_train"]["graph"]
            asp = [b for b in g.ie.mid if type(b).__name__ == "ASPPT"][0]
            stale = (asp.cat.only16, g.s1f.cat.only16)
            grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
            return float(total), grads, stale
        finally:
            T.FP16_ONLY_STORES[0] = True

    l1, g1, st1 = step(True)
    l0, g0, st0 = step(False)
    assert st1 == (True, True) and st0 == (False, False), (st1, st0)
    assert l1 == l0
    assert g1.keys() == g0.keys() and len(g1) > 0
    for n in g1:
        assert torch.equal(g1[n], g0[n]), n
