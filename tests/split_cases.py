"""What the GPU tests of the fp32 split forms share (test_gpu_split_conv.py,
_split_regs.py, _split_w64.py, _ring_w64.py, _ring_lds_split.py): model
handles with the switches a test wants, the float64 oracle of a model forward,
the seeded inputs of the op-level cases and the exact-path runner.

A plain module, imported by those files; every case table, seed, shape and
tolerance stays in the file that uses it, or here when two files use it.
"""
import torch
import torch.nn.functional as F

from oracle import net as onet

DEV = "cuda:0"

# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------
# the ops of the split-fp16 region (form 1 of upr_model_op_forms)
REGION = ["ie_net." + n for n in (
    "enc2.conv1", "enc2.conv2", "enc3.conv1", "enc3.conv2", "bottleneck.0.conv1", "bottleneck.0.conv2",
    "bottleneck.1.conv1", "bottleneck.1.conv2", "dec3.up", "dec3.conv.0", "dec3.conv.3")]


def regs_ops(H, W):
    """The ops that run split in registers at an H x W input: the row ring takes
    outputs of at least 4 rows and 16 columns (the FAM scales are H, H/4, H/16)."""
    names = ["ie_net.dec1.conv.0", "ie_net.dec1.conv.3", "ie_net.residual_head"]
    for p, sh in (("scale1.2", 0), ("scale2.3", 2), ("scale3.3", 4)):
        h, w = H, W
        for _ in range(sh // 2):
            h, w = (h // 2) // 2, (w // 2) // 2
        if h >= 4 and w >= 16:
            names += [p + ".branch34_conv1", p + ".fusion.h3x", p + ".fusion.h4"]
    return sorted(names)


def make_sd(pre, aspp, seed=0):
    from models.model import UP_Retinex
    torch.manual_seed(seed)
    return {k: v.detach().clone() for k, v in UP_Retinex(use_preact=pre, use_aspp=aspp).eval().state_dict().items()}


SWITCHES = {"split": "UPR_FP32_SPLIT", "regs": "UPR_FP32_SPLIT_REGS", "w64": "UPR_FP32_SPLIT_W64"}


def make_handle(sd, pre, aspp, monkeypatch, dtype=torch.float32, **switches):
    """A handle created with the given on / off switches (split=, regs=, w64=)
    set to 1 / 0 through the test's monkeypatch; the others stay as they are.
    They are read when the handle is created."""
    from upr.runtime import ModelHandle
    for name, on in switches.items():
        monkeypatch.setenv(SWITCHES[name], "1" if on else "0")
    return ModelHandle(sd, pre, aspp, dtype, torch.device(DEV))


def fwd(h, x):
    out = h.forward(x)
    torch.cuda.synchronize()
    return [o.clone() for o in out]


_F64 = {}


def oracle_f64(sd, x, pre, aspp, key):
    """The float64 forward of the reference network, computed once per (pre,
    aspp, key): key names the state dict and input (the tests use seed 0 / seed
    11 and pass the shape)."""
    key = (pre, aspp, key)
    if key not in _F64:
        sd64 = {k: (v.double() if torch.is_floating_point(v) else v) for k, v in sd.items()}
        with torch.no_grad():
            _F64[key] = [o.double() for o in onet.forward(sd64, x.double(), pre, aspp)]
    return _F64[key]


# ---------------------------------------------------------------------------
# op level
# ---------------------------------------------------------------------------
def nhwc(t):
    return None if t is None else t.permute(0, 2, 3, 1).contiguous().to(DEV)


# the row ring (3x3, stride 1, pad 1, Cin 32): test_gpu_split_regs.py and test_gpu_ring_lds_split.py
RING_CASES = [
    # B, H, W, Cout, relu, residual
    (1, 4, 16, 32, False, False),   # the smallest unit the ring takes
    (2, 6, 40, 32, True, False),    # partial last step, partial second strip, image boundary
    (2, 9, 72, 64, True, False),    # four channel tiles (W_lo from LDS), three strips
    (2, 8, 48, 32, False, True),    # residual landing zone
]


def ring_inputs(case, scale, seed=4321):
    B, H, W, Cout, relu, res = case
    Cin = 32
    g = torch.Generator().manual_seed(seed + 7 * Cout + H + 3 * W)
    x = F.relu(torch.randn(B, Cin, H, W, generator=g)) * scale
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    b = torch.randn(Cout, generator=g) * scale
    ref = F.conv2d(x.double(), w.double(), b.double(), 1, 1)
    r = None
    if res:
        r = torch.randn(ref.shape, generator=g) * scale
        ref = ref + r.double()
    if relu:
        ref = F.relu(ref)
    return x, w, b, r, ref.permute(0, 2, 3, 1)


class WsplitCases:
    """The weights-split-once op (upr_conv2d_nhwc_wsplit) over one file's case
    table.  A case is (B, H, W, Cin, Cout, stride, [pad, dil,] relu, residual
    after the ReLU, second segment (H2, W2, C2, stride2) or None), 3x3, pad =
    dil = 1 where the table leaves them out.  seed(B, H, W, Cin, Cout) gives
    the file's generator seed; label starts its printed lines."""

    def __init__(self, cases, seed, label):
        self.cases, self.seed, self.label = cases, seed, label
        self._inputs = {}

    def geometry(self, name):
        B, H, W, Cin, Cout, stride, *pad_dil, relu, res, seg2 = self.cases[name]
        pad, dil = pad_dil or (1, 1)
        return B, H, W, Cin, Cout, stride, pad, dil, relu, res, seg2

    def inputs(self, name, scale=1.0):
        """Seeded tensors and the float64 reference of one case (computed once, never changed)."""
        if (name, scale) in self._inputs:
            return self._inputs[(name, scale)]
        B, H, W, Cin, Cout, stride, pad, dil, relu, res, seg2 = self.geometry(name)
        g = torch.Generator().manual_seed(self.seed(B, H, W, Cin, Cout))
        x = F.relu(torch.randn(B, Cin, H, W, generator=g)) * scale
        w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
        b = torch.randn(Cout, generator=g) * scale
        ref = F.conv2d(x.double(), w.double(), b.double(), stride, pad, dil)
        x2 = w2 = None
        if seg2 is not None:
            H2, W2, C2, s2 = seg2
            x2 = F.relu(torch.randn(B, C2, H2, W2, generator=g)) * scale
            w2 = torch.randn(Cout, C2, generator=g) / C2 ** 0.5
            ref = ref + F.conv2d(x2.double(), w2.double().view(Cout, C2, 1, 1), None, s2, 0)
        if relu:
            ref = F.relu(ref)
        r = None
        if res:
            r = torch.randn(ref.shape, generator=g) * scale
            ref = ref + r.double()
        self._inputs[(name, scale)] = (x, w, b, r, x2, w2, ref.permute(0, 2, 3, 1).contiguous())
        return self._inputs[(name, scale)]

    def run_wsplit(self, name, scale=1.0, ovf=None, poke=None):
        """One upr_conv2d_nhwc_wsplit call (UPR_W64_RING / UPR_RING_SPLIT_LDS are read at the
        call) -> (y, the kernel that ran)."""
        from upr import runtime
        _, _, _, _, Cout, stride, pad, dil, relu, _, seg2 = self.geometry(name)
        x, w, b, r, x2, w2, _ = self.inputs(name, scale)
        xd = nhwc(x)
        if poke is not None:
            xd[poke] = 70000.0
        blob = runtime.pack_split_w(runtime.pack_conv_weight(w), 3, 3, w2).to(DEV)
        y = runtime.conv2d_nhwc_wsplit(xd, blob, Cout, b.to(DEV), 3, 3, stride, pad, dil, residual=nhwc(r), relu=relu,
                                       x2=nhwc(x2), stride2=seg2[3] if seg2 else 1, overflow=ovf)
        return y, runtime.last_wsplit_kernel()

    def run_exact(self, name, scale=1.0):
        """The same op on the exact fp32 kernels: the conv (+ bias, ReLU when there is
        no second segment), the 1x1 segment as its own conv, the rest in torch."""
        from upr import runtime
        _, _, _, _, _, stride, pad, dil, relu, _, seg2 = self.geometry(name)
        x, w, b, r, x2, w2, _ = self.inputs(name, scale)
        wd, bd = runtime.pack_conv_weight(w).to(DEV), b.to(DEV)
        if seg2 is None:
            y = runtime.conv2d_nhwc(nhwc(x), wd, bd, 3, 3, stride, pad, dil, relu=relu)
        else:
            y = runtime.conv2d_nhwc(nhwc(x), wd, bd, 3, 3, stride, pad, dil)
            y = y + runtime.conv2d_nhwc(nhwc(x2), w2.contiguous().to(DEV), None, 1, 1, seg2[3], 0, 1)
            if relu:
                y = F.relu(y)
        if r is not None:
            y = y + nhwc(r)
        return y

    def errors(self, name, scale, kernel=None):
        """(error of the split op, error of the exact kernels) against float64;
        kernel: the one that must have run ("ring" / "tile"), where the test pins it."""
        refn = self.inputs(name, scale)[-1]
        ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
        y16, ran = self.run_wsplit(name, scale, ovf)
        y32 = self.run_exact(name, scale)
        torch.cuda.synchronize()
        if kernel is not None:
            assert ran == kernel, f"{name}: ran on {ran}, expected {kernel}"
        assert int(ovf.item()) == 0
        assert y16.shape == refn.shape
        e32 = (y32.double().cpu() - refn).abs().max().item()
        e16 = (y16.double().cpu() - refn).abs().max().item()
        print(f"{self.label} {kernel or ''} {name} x{scale:g}: max|y| {refn.abs().max().item():.4g}  fp32 err {e32:.3e}  "
              f"wsplit err {e16:.3e}  ratio {e16 / max(e32, 1e-300):.2f}")
        return e16, e32
