"""Self-check of the float64 op reference oracle/fam_ops.py (numpy) against
torch autograd in double: both sides are float64, so they agree to 1e-12
relative (of the largest reference magnitude).  The channel maximum is
torch.max(dim) as the reference model has it: on a tie its gradient goes whole
to the first maximum, where amax would split it; the tied cases below tell
the two apart, and the last test holds oracle/net.py::fam to the same rule."""
import numpy as np
import pytest
import torch

from oracle import fam_ops as O
from oracle import net as onet

REL = 1e-12


def _agree(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), b.detach().double().numpy()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b).max()
    tol = REL * max(np.abs(b).max(), 1e-300)
    assert err <= tol, f"{what}: max|d| {err:.3e} > {tol:.3e}"


def _t(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).requires_grad_(grad)


def _attention_inputs(B, HW, C, tied, seed):
    rng = np.random.default_rng(seed)
    o = np.maximum(rng.standard_normal((B, HW, C)), 0.0)  # a ReLU's output: about half exact zeros
    if tied:
        # small integers: most pixels have their maximum on several channels at once
        o = rng.integers(0, 3, (B, HW, C)).astype(np.float64)
    ca = np.ones((B, C)) if tied else rng.uniform(0.05, 0.95, (B, C))
    if C > 2 and not tied:
        ca[:, 1], ca[:, 2] = 0.0, -0.3
    return (o, ca, rng.standard_normal((B, HW)), rng.standard_normal((B, HW, C)),
            rng.standard_normal((B, HW, 2)))


@pytest.mark.parametrize("B,HW,C,tied", [(2, 13, 5, False), (1, 7, 32, False), (2, 29, 4, True), (1, 40, 32, True),
                                         (3, 5, 1, False)])
def test_attention_matches_autograd_double(B, HW, C, tied):
    o, ca, s_pre, g, g_m = _attention_inputs(B, HW, C, tied, 11)
    ot, cat, st = _t(o, True), _t(ca, True), _t(s_pre, True)
    o2t = ot * cat[:, None, :]
    mt = torch.stack([o2t.mean(-1), torch.max(o2t, dim=-1)[0]], -1)
    sat = torch.sigmoid(st)
    outt = o2t * sat[..., None]
    ((outt * _t(g)).sum() + (mt * _t(g_m)).sum()).backward()

    o2, m = O.ca_apply(o, ca)
    sa, out = O.sa_apply(o2, s_pre)
    _agree(o2, o2t, "o2")
    _agree(m, mt, "m")
    _agree(sa, sat, "sa")
    _agree(out, outt, "out")
    g_o2, g_spre = O.sa_bwd(g, o2, sa)
    g_o, g_ca = O.ca_bwd(g_o2, g_m, o, o2, ca)
    _agree(g_spre, st.grad, "g_spre")
    _agree(g_o, ot.grad, "g_o")
    _agree(g_ca, cat.grad, "g_ca")
    if tied:
        tie = (o2 == o2.max(-1, keepdims=True)).sum(-1) > 1
        assert tie.mean() > 0.3
        # amax's even split is a different gradient on these inputs
        o_a = _t(o, True)
        (torch.amax(o_a * cat.detach()[:, None, :], dim=-1) * _t(g_m[..., 1])).sum().backward()
        o_m = _t(o, True)
        (torch.max(o_m * cat.detach()[:, None, :], dim=-1)[0] * _t(g_m[..., 1])).sum().backward()
        assert (o_a.grad - o_m.grad).abs().max() > 0.1


def test_ca_bwd_first_maximum_and_first_nan():
    """The max route lands on the first maximum, or the first NaN."""
    C = 8
    o2 = np.zeros((1, 4, C))
    o2[0, 1, [2, 6]] = 5.0
    o2[0, 2] = -np.inf
    o2[0, 3, 1], o2[0, 3, 4], o2[0, 3, 6] = 9.0, np.nan, np.nan
    g_m = np.stack([np.zeros((1, 4)), np.arange(1.0, 5.0)[None]], -1)
    g_o, _ = O.ca_bwd(np.zeros((1, 4, C)), g_m, np.zeros((1, 4, C)), o2, np.ones((1, C)))
    want = np.zeros((1, 4, C))
    want[0, 0, 0], want[0, 1, 2], want[0, 2, 0], want[0, 3, 4] = 1.0, 2.0, 3.0, 4.0
    assert np.array_equal(g_o, want)
    m = O.ca_apply(o2, np.ones((1, C)))[1]
    assert np.array_equal(m[0, :3, 1], [0.0, 5.0, -np.inf]) and np.isnan(m[0, 3, 1])


def test_pool_bwd_matches_autograd_double():
    B, HW, C = 2, 11, 6
    rng = np.random.default_rng(12)
    pre = rng.standard_normal((B, HW, C))
    g_o, g_pool = rng.standard_normal((B, HW, C)), rng.standard_normal((B, C))
    pt = _t(pre, True)
    ot = torch.relu(pt)
    ((ot * _t(g_o)).sum() + (ot.mean(1) * _t(g_pool)).sum()).backward()
    _agree(O.pool_bwd(g_o, g_pool, ot.detach().numpy()), pt.grad, "pool_bwd")


def _tail_inputs(B, H, W, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0, 1, (B, 3, H, W)), rng.standard_normal((B, H, W)), 2 * rng.standard_normal((B, H, W, 3)),
            rng.standard_normal((B, 3, H, W)), rng.standard_normal((B, 3, H, W)), rng.standard_normal((B, H, W)))


@pytest.mark.parametrize("with_refl,with_illu", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (3, 5, 7)])
def test_retinex_matches_autograd_double(B, H, W, with_refl, with_illu):
    x, r, o, g_enh, g_refl, g_illu = _tail_inputs(B, H, W, 13)
    rt, ot = _t(r, True), _t(o, True)
    xt = _t(x)
    illu_t = torch.sigmoid(xt.mean(1) + rt)
    refl_t = xt / (illu_t[:, None] + 1e-6)
    e_t = torch.sigmoid(ot)
    ec = e_t.permute(0, 3, 1, 2)
    enh_t = refl_t * ec + (1 - refl_t) * ec * ec
    loss = (enh_t * _t(g_enh)).sum()
    if with_refl:
        loss = loss + (refl_t * _t(g_refl)).sum()
    if with_illu:
        loss = loss + (illu_t * _t(g_illu)).sum()
    loss.backward()

    illu = O.head_fwd(x, r)
    e, refl, enh = O.retinex_fwd(x, illu, o)
    for name, a, b in (("illu", illu, illu_t), ("e", e, e_t), ("refl", refl, refl_t), ("enh", enh, enh_t)):
        _agree(a, b, name)
    g_o, g_r = O.retinex_bwd(x, illu, e, refl, g_enh, g_refl if with_refl else None, g_illu if with_illu else None)
    _agree(g_o, ot.grad, "g_o")
    _agree(g_r, rt.grad, "g_r")


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 4, 6)])
def test_enhance_matches_autograd_double(B, H, W):
    _, _, o, g_enh, g_refl, _ = _tail_inputs(B, H, W, 14)
    refl = np.random.default_rng(15).uniform(0, 3, (B, 3, H, W))
    ft, ot = _t(refl, True), _t(o, True)
    e_t = torch.sigmoid(ot)
    ec = e_t.permute(0, 3, 1, 2)
    enh_t = ft * ec + (1 - ft) * ec * ec
    (enh_t * _t(g_enh)).sum().backward()
    e, enh = O.enhance_fwd(refl, o)
    _agree(e, e_t, "e")
    _agree(enh, enh_t, "enh")
    g_o, g_rf = O.enhance_bwd(e, refl, g_enh)
    _agree(g_o, ot.grad, "g_o")
    _agree(g_rf, ft.grad, "g_refl")


def test_helpers_match_torch_double():
    rng = np.random.default_rng(16)
    x, out0 = rng.standard_normal((2, 37, 6)), rng.standard_normal((2, 6))
    _agree(O.pixel_sum(x, 0.25), _t(x).sum(1) * 0.25, "pixel_sum")
    _agree(O.pixel_sum(x, 1 / 37, out0), _t(x).sum(1) / 37 + _t(out0), "pixel_sum accumulated")
    v, y0 = rng.standard_normal((2, 6)), rng.standard_normal((2, 5, 6))
    _agree(O.broadcast(v, 0.5, 5), (_t(v) * 0.5)[:, None, :].expand(2, 5, 6), "broadcast")
    _agree(O.broadcast(v, 0.5, 5, y0), (_t(v) * 0.5)[:, None, :] + _t(y0), "broadcast accumulated")
    a, b = rng.standard_normal(101) * 3, rng.standard_normal(101)
    at = _t(a, True)
    s = torch.sigmoid(at)
    s.backward(_t(b))
    _agree(O.sigmoid(a), s, "sigmoid")
    _agree(O.sigmoid_bwd(b, O.sigmoid(a)), at.grad, "sigmoid backward")
    _agree(O.add(a, b), _t(a) + _t(b), "add")
    _agree(O.scale(a, -1.75), _t(a) * -1.75, "scale")


def _splitmix64(seed, i):
    """Python-integer splitmix64 of (seed, index), masked to 64 bits."""
    M = (1 << 64) - 1
    z = (seed + 0x9E3779B97F4A7C15 * (i + 1)) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


@pytest.mark.parametrize("seed", [0, 0x1234567, (1 << 64) - 3])
def test_dropout_mask_is_splitmix64(seed):
    """The numpy uint64 hash equals arbitrary-precision integer arithmetic;
    the mask keeps u >= p, and the kept values are a / (1 - p)."""
    n = 300
    u = O.hash_uniform(seed, n)
    want = np.array([(_splitmix64(seed, i) >> 40) / 2.0 ** 24 for i in range(n)])
    assert np.array_equal(u, want) and u.min() >= 0 and u.max() < 1
    for p in (0.0, 0.1, 0.5):
        mask = O.dropout_mask(n, p, seed)
        assert np.array_equal(mask, (want >= np.float32(p)).astype(np.uint8))
        a = np.linspace(-2, 2, n)
        _agree(O.dropout(a, mask, p), _t(a) * _t(mask.astype(np.float64)) / (1 - float(np.float32(p))), f"dropout {p}")
    assert O.dropout_mask(n, 0.0, seed).all()


def _fam_sd(ci, co, rng):
    sq = max(co // 4, 1)
    shapes = {"branch1": (co, ci, 1, 1), "branch2_conv": (co, ci, 1, 1), "branch3_conv1": (co, ci, 3, 3),
              "branch3_conv2": (co, co, 3, 3), "branch4_conv1": (co, ci, 3, 3), "branch4_conv2": (co, co, 3, 3),
              "fusion": (co, 4 * co, 1, 1), "channel_attention.1": (sq, co, 1, 1),
              "channel_attention.3": (co, sq, 1, 1), "spatial_attention.0": (1, 2, 7, 7)}
    sd = {}
    for k, s in shapes.items():
        sd[f"m.{k}.weight"] = torch.from_numpy(rng.standard_normal(s) * 0.3)
        sd[f"m.{k}.bias"] = torch.from_numpy(rng.standard_normal(s[0]) * 0.1)
    return sd


def test_net_fam_tie_gradient_goes_to_first_index():
    """oracle/net.py::fam with channels 1 and 4 of the attended tensor equal
    everywhere (and the maximum at many pixels): its gradients equal those of
    the same forward with the channel maximum gathered at the first maximal
    index.  The twins are the same function of x, so x's gradient is the same
    however the max route is shared between them; the fusion conv's rows 1
    and 4 are what tell: the whole route lands on row 1, where an even split
    among tied maxima (amax) gives both rows the same gradient."""
    rng = np.random.default_rng(17)
    ci, co = 3, 6
    sd0 = _fam_sd(ci, co, rng)
    for k in ("m.fusion", "m.channel_attention.3"):
        sd0[k + ".weight"][4] = sd0[k + ".weight"][1]
        sd0[k + ".bias"][4] = sd0[k + ".bias"][1]
    # the twins large (fusion bias 3) and nearly unattenuated (attention bias 3): often the maximum
    sd0["m.fusion.bias"][1] = sd0["m.fusion.bias"][4] = 3.0
    sd0["m.channel_attention.3.bias"][1] = sd0["m.channel_attention.3.bias"][4] = 3.0
    x0 = rng.standard_normal((2, ci, 9, 8))
    g = torch.from_numpy(rng.standard_normal((2, co, 9, 8)))
    F = torch.nn.functional

    def explicit(sd, xe):
        """fam's forward, the maximum taken by a gather at the first maximal index."""
        def conv(name, t, **kw):
            return onet._conv(sd, "m." + name, t, **kw)
        b1 = conv("branch1", xe)
        b2 = conv("branch2_conv", F.max_pool2d(xe, 3, 1, 1))
        b3 = conv("branch3_conv2", F.relu(conv("branch3_conv1", xe, padding=1)), padding=1)
        b4 = conv("branch4_conv2", F.relu(conv("branch4_conv1", xe, padding=1)), padding=2, dilation=2)
        out = F.relu(conv("fusion", torch.cat([b1, b2, b3, b4], 1)))
        ca = torch.sigmoid(conv("channel_attention.3",
                                F.relu(conv("channel_attention.1", out.mean((2, 3), keepdim=True)))))
        out = out * ca
        first = torch.from_numpy(np.argmax(out.detach().numpy(), axis=1))[:, None]
        tied = (out.detach() == out.detach().amax(1, keepdim=True)).sum(1) > 1
        assert torch.equal(out[:, 1], out[:, 4]) and tied.float().mean() > 0.2
        assert (first[:, 0] == 1).float().mean() > 0.2 and not (first == 4).any()  # never the later twin
        m = torch.cat([out.mean(1, keepdim=True), out.gather(1, first)], 1)
        return out * torch.sigmoid(conv("spatial_attention.0", m, padding=3))

    def run(forward):
        sd = {k: v.clone().requires_grad_(True) for k, v in sd0.items()}
        x = _t(x0, True)
        y = forward(sd, x)
        (y * g).sum().backward()
        return y.detach(), x.grad, sd["m.fusion.weight"].grad, sd["m.fusion.bias"].grad

    got = run(lambda sd, x: onet.fam(sd, "m", x))
    want = run(explicit)
    for name, a, b in zip(("forward", "input gradient", "fusion weight gradient", "fusion bias gradient"), got, want):
        _agree(a.numpy(), b, "fam on tied channels: " + name)
    # the route is not shared: rows 1 and 4 differ by the whole max-route gradient
    assert (want[3][1] - want[3][4]).abs() > 1e-3
