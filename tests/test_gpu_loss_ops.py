"""Op-level parity of the loss kernels (csrc/train_loss.hip) and of
upr_t_sqsum (csrc/train_optim.hip) against the float64 reference
oracle/loss_ops.py (run with `-m gpu`).  Every entry is called through ctypes
(upr._lib.lib()) on inputs made on the CPU (tests/loss_ops_cases.py), one op at
a time: no op reads another kernel's output.

Shapes.  upr_t_loss_pixel_p runs loss_pass1_band_kernel when the patch is a
power of two <= 64 dividing H and W (256 columns an x-block, a patch = adjacent
lanes of a wave), else loss_pass1_kernel (per-pixel fp64 atomics); the generic
pass 1, pass 2 and the edge-density passes split HW into clamp(HW / 4096, 1,
128) chunks.  loss_ops_cases.PIXEL_SHAPES names what each shape reaches.  Each
shape runs every term alone (one of w_exp, w_col, w_spa, w_dec, w_smooth = 1,
the rest 0), so that a small term's gradient is bounded by its own size, and
once mixed with non-default weights and module arguments.

Input conditions (asserted on the float64 reference before the device is
touched, and in test_cpu_loss_ops_oracle.py): exposure patches on both sides of
the target and >= 1e-3 from it; no Sobel magnitude within 1e-5 of the
edge-density threshold; the dynamic smooth weight reaches both clamps.

Tolerances (tests/op_parity.py).
  * _within_restated: the kernel's error against float64 within 4x the error
    of the same formula in plain fp32 torch ops on the CPU (for the pixel
    terms: oracle/train.py at float32, gradients by autograd), at least half
    an ulp of the largest |reference|, and under 1e-4 max|ref| + 1e-6.  Each
    scalar term is held to it on its own.
  * _within_ulp at 1 ulp: vgg_norm, vgg_norm_bwd, add_real (a quotient or a
    product, then one add; the addends have one sign, so that the first
    rounding is not magnified by cancellation); 2 ulp: loss_total's terms[7].
  * bit-equal: the edge-density share, scale_acc, every zero the header or the
    mathematics promises (absent terms, remainder rows and columns, ties of
    the illumination differences, G at |Ze| = 0), the three channels of the
    exposure gradient, G of upr_t_freq against upr_t_freq_p(1, 0.5), every
    sentinel (frames around outputs, terms[5..7], the workspace's tail,
    outputs of refused calls).
  * 1e-12 relative: upr_t_sqsum as a double (only the order of the fp64
    additions differs).

Measured on the MI355X (profiles/loss_ops_gpu_tests_v1.log): max |error|
against float64 in ulp of the case's largest |reference|, the worst case of
each group; "used" is the worst kernel error / allowed error over all cases (1
would fail).  The restatement of exposure (one patch), colour and decoupling
is tens to hundreds of ulp off (differences of fp32 means); the kernels
accumulate in fp64.

  group (calls)                            restatement   kernel   used
  term exposure (74)                          194.21       7.54    0.24
  term smoothness (76)                          1.23       0.99    0.28
  term colour (74)                             33.03       0.48    0.13
  term spatial (74)                             1.29       0.44    0.20
  term decouple (74)                          291.32       0.46    0.12
  smooth weight, terms[8] (74)                  0.55       0.45    0.20
  g_enh, exposure alone (9)                     0.37       0.37    0.19
  g_enh, colour alone (9)                      12.77       5.43    0.25
  g_enh, spatial alone (9)                      1.74       1.48    0.27
  g_illu, smoothness alone (9)                  2.13       2.01    0.29
  g_illu, decoupling alone (9)                832.63       2.69    0.13
  g_refl, decoupling alone (9)                358.83       3.23    0.11
  g_enh / g_illu / g_refl, mixed (9)     1.93 / 1.98 / 378.54   2.28 / 2.75 / 3.30   0.38
  the same, dynamic smooth weight (12)   1.17 / 4.18 / 122.04   1.48 / 3.08 / 2.63   0.40
  the same, upr_t_loss_pixel defaults (8) 0.95 / 1.74 / 282.25  1.25 / 1.67 / 3.03   0.33
  g_illu on a piecewise-constant plane (2)      1.90       1.39    0.18
  texture 'tv' (9)                              1.22       0.81    0.40
  freq sum (12)                                 1.22       0.63    0.15
  freq G (3)                                    1.62       2.58    0.40
  mse value / g (8 / 4)                     0.70 / 1.19  0.03 / 1.19   0.25
  mse16 value / g (8 / 4)                   1.16 / 0.50  0.00 / 0.50   0.25

  The exposure term's 7.54 ulp is the 2 x 2 image (4 pixels: the fp32 gray of
  each pixel is not averaged away; restatement 14.54); every other shape is
  under 0.7 ulp.  vgg_norm: 1 ulp at most, 97% of the elements bit-equal;
  vgg_norm_bwd: 1 ulp at most, 78% bit-equal (the quotient is rounded before
  the add); add_real, loss_total: 0 ulp; sqsum: 2.5e-15 relative at n = 2^19 +
  5.  Every bit-equal check held.  114 tests in 3.2 s; the slowest is 0.18 s
  (the first pixel-loss call), the 2^20 + 3 element MSE takes 0.10 s.

One miss, fixed in the kernels.  On a 2 x 2 image the reflect pad mirrors every
Sobel tap onto its opposite, both derivatives are 0 and 'edge_density' counts
nothing.  edge_at and texture_kernel summed gy as -a - 2b - c + a + 2b + c,
which leaves rounding noise of about 1e-8 instead of 0, and the count of
e > 1.5 mean e then counted noise (oracle/train.py's conv2d does the same in
float64: that is why oracle/loss_ops.py::sobel_magnitude pairs the taps).  gy
now adds each tap next to its mirror tap, as gx already did: exactly 0 on a
2-sample axis, the same operations elsewhere.  Also: upr_t_mse with n == 0
added 0 / 0 into acc; it now returns UPR_OK untouched, as upr_t_mse16 does.
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import loss_ops_cases as K
from conftest import has_gpu
from op_parity import DEV, P, SENT, _within_restated, _within_ulp
from oracle import loss_ops as O
from oracle import train as T

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a ROCm device")]

PAD = 64          # sentinel elements on either side of an output
WS_TAIL = 4096    # sentinel bytes after the workspace
WS_FILL = 0xA5
TERM_NAMES = ("exposure", "smoothness", "colour", "spatial", "decouple")


def _lib():
    from upr import _lib as L
    return L, L.lib(), torch.cuda.current_stream().cuda_stream


def _tt(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64))


class Framed:
    """n elements on the device inside a buffer of n + 2 PAD, everything the
    sentinel: .ptr is the first inner element, .get() the inner part on the
    CPU after checking that the frame still holds the sentinel."""

    def __init__(self, shape, dtype=torch.float32, fill=SENT):
        self.shape, self.n, self.fill = tuple(shape), int(np.prod(shape)), fill
        self.buf = torch.full((self.n + 2 * PAD,), fill, dtype=dtype, device=DEV)
        self.ptr = self.buf.data_ptr() + PAD * self.buf.element_size()

    def set(self, t):
        self.buf[PAD:PAD + self.n] = t.reshape(-1).to(DEV)
        return self

    def get(self, what="output"):
        b = self.buf.cpu()
        for part in (b[:PAD], b[PAD + self.n:]):
            assert torch.equal(part, torch.full_like(part, self.fill)), f"{what}: wrote outside its buffer"
        return b[PAD:PAD + self.n].view(self.shape)

    def untouched(self):
        return torch.equal(self.buf, torch.full_like(self.buf, self.fill))


# ---------------------------------------------------------------------------
# pixel loss
# ---------------------------------------------------------------------------
def _params(L, shape, prm):
    p = dict(O.DEFAULT_PARAMS)
    p.update(prm)
    return L.UprLossParams(shape[3], p["base_exposure"], p["smooth_lambda"], p["smooth_alpha"], p["decouple_lambda"],
                           1.0, 0.5, int(p["dynamic_smooth"]), shape[4])


def _run_pixel(d, shape, weights, w_smooth, texture, prm, default_entry=False):
    """One upr_t_loss_pixel_p (or upr_t_loss_pixel) call on d: terms and the
    gradients start as sentinels inside sentinel frames, the workspace is
    exactly upr_t_loss_workspace_p bytes followed by a sentinel tail."""
    L, lib, st = _lib()
    B, H, W, patch, CI = shape
    nbytes = lib.upr_t_loss_workspace_p(B, H, W, patch)
    assert nbytes > 0
    ws = torch.full((nbytes + WS_TAIL,), WS_FILL, dtype=torch.uint8, device=DEV)
    names = ("low", "enh", "illu", "refl")
    dev = {k: d[k].to(DEV) for k in names}
    terms, g_enh, g_illu, g_refl = Framed((9,)), Framed((B, 3, H, W)), Framed((B, CI, H, W)), Framed((B, 3, H, W))
    args = [*(P(dev[k]) for k in names), B, H, W, P(ws), terms.ptr, g_enh.ptr, g_illu.ptr, g_refl.ptr, 1,
            *weights, w_smooth, texture]
    if default_entry:
        rc = lib.upr_t_loss_pixel(*args, st)
    else:
        cp = _params(L, shape, prm)
        rc = lib.upr_t_loss_pixel_p(*args, ctypes.byref(cp), st)
    torch.cuda.synchronize()
    assert rc == 0, rc
    tail = ws[nbytes:].cpu()
    assert torch.equal(tail, torch.full_like(tail, WS_FILL)), "wrote past upr_t_loss_workspace_p bytes"
    t = terms.get("terms")
    assert torch.equal(t[5:8], torch.full((3,), SENT)), "terms[5..7] are not upr_t_loss_pixel's to write"
    for k in names:
        assert torch.equal(dev[k].cpu(), d[k]), f"{k}: an input was written"
    return SimpleNamespace(terms=t, g_enh=g_enh.get("g_enh"), g_illu=g_illu.get("g_illu"), g_refl=g_refl.get("g_refl"))


@functools.lru_cache(maxsize=None)
def _pixel_ref(shape, weights, w_smooth, texture, prm_items):
    """(float64 reference, plain-fp32 restatement) of one call: computed once, shared, never written."""
    d = K.pixel_inputs(*shape)
    prm = dict(prm_items, patch=shape[3])
    return tuple(O.pixel_terms(d["low"], d["enh"], d["illu"], d["refl"], weights, prm, w_smooth, texture, dt)
                 for dt in (torch.float64, torch.float32))


def _check_pixel(out, ref, group, tag):
    (t64, wsm64, *g64), (t32, wsm32, *g32) = ref
    for k, name in enumerate(TERM_NAMES):
        _within_restated(f"term {name} | {tag}", out.terms[k], t64[k], _tt(t32[k]))
    _within_restated(f"smooth weight | {tag}", out.terms[8], np.float64(wsm64), _tt(wsm32))
    for name, dev, a, b in zip(("g_enh", "g_illu", "g_refl"), (out.g_enh, out.g_illu, out.g_refl), g64, g32):
        _within_restated(f"{name} {group} | {tag}", dev, a, _tt(b))


def _zero(t):
    return not t.numpy().any()


@pytest.mark.parametrize("wname", list(K.WEIGHTINGS))
@pytest.mark.parametrize("shape", K.PIXEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_pixel(shape, wname):
    """upr_t_loss_pixel_p: terms[0..4], terms[8] and the three gradients of
    every term alone and of the mixed weighting against float64; the zeros
    that must be exact; the contracts of _run_pixel."""
    B, H, W, patch, CI = shape
    d = K.check_pixel_inputs(*shape)
    weights, w_smooth, prm = K.WEIGHTINGS[wname]
    prm = dict(prm, dynamic_smooth=0)
    ref = _pixel_ref(shape, weights, w_smooth, 0, tuple(sorted(prm.items())))
    out = _run_pixel(d, shape, weights, w_smooth, 0, prm)
    _check_pixel(out, ref, wname, f"{wname} {shape}")
    assert float(out.terms[8]) == O.f32(w_smooth), "dynamic_smooth = 0: terms[8] is w_smooth"
    w_exp, w_col, w_spa, w_dec = weights
    if not (w_exp or w_col or w_spa):
        assert _zero(out.g_enh), "g_enh without exposure, colour and spatial weights"
    if not w_dec:
        assert _zero(out.g_refl), "g_refl without the decoupling weight"
        if not w_smooth:
            assert _zero(out.g_illu), "g_illu without smoothness and decoupling weights"
    if wname == "exp":
        g = out.g_enh
        assert torch.equal(g[:, 0], g[:, 1]) and torch.equal(g[:, 0], g[:, 2]), "exposure gradient differs by channel"
        ph, pw = (H // patch) * patch, (W // patch) * patch
        assert _zero(g[:, :, ph:]) and _zero(g[:, :, :, pw:]), "exposure gradient on the remainder rows / columns"
        inner = g[:, :, :ph, :pw]
        assert bool((inner != 0).all()), "every pooled pixel has an exposure gradient (|P - T| >= 1e-3)"
        if B * (H // patch) * (W // patch) > 1:
            assert bool((inner > 0).any()) and bool((inner < 0).any()), "sign(P - T) goes both ways"


@pytest.mark.parametrize("w_smooth", K.DYNAMIC_W_SMOOTH)
@pytest.mark.parametrize("texture", [0, 1])
@pytest.mark.parametrize("shape", K.DYNAMIC_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_pixel_dynamic_smooth(shape, texture, w_smooth):
    """dynamic_smooth = 1 with both texture methods: w_smooth = 0.05 / 1 / 10
    ends at the 0.1 clamp, unclamped and at the 5.0 clamp; terms[8] and the
    gradients (g_illu carries the weight) against float64."""
    d = K.check_pixel_inputs(*shape)
    K.check_dynamic_weights(d["low"])
    weights, _, prm = K.WEIGHTINGS["mixed"]
    prm = dict(prm, dynamic_smooth=1)
    ref = _pixel_ref(shape, weights, w_smooth, texture, tuple(sorted(prm.items())))
    out = _run_pixel(d, shape, weights, w_smooth, texture, prm)
    _check_pixel(out, ref, f"dynamic t{texture}", f"dynamic texture={texture} w_smooth={w_smooth} {shape}")
    got = float(out.terms[8])
    if w_smooth == K.DYNAMIC_W_SMOOTH[0]:
        assert got == O.f32(0.1)
    elif w_smooth == K.DYNAMIC_W_SMOOTH[2]:
        assert got == 5.0
    else:
        assert 0.1 < got < 5.0


@pytest.mark.parametrize("shape", [(1, 32, 272, 16, 1), (1, 71, 123, 12, 3)], ids=lambda s: "x".join(map(str, s)))
def test_loss_pixel_illumination_ties(shape):
    """sign(0) = 0 of the smoothness gradient: a constant illumination gives
    terms[1] = 0 and g_illu = 0 everywhere; a piecewise-constant one (a
    vertical step on plane 0, a horizontal one on the last plane) gives 0
    inside the pieces and a gradient on the two lines along each step."""
    B, H, W, patch, CI = shape
    d = dict(K.check_pixel_inputs(*shape))
    weights, w_smooth, prm = K.WEIGHTINGS["smooth"]
    prm = dict(prm, dynamic_smooth=0)
    d["illu"] = torch.full((B, CI, H, W), 0.4)
    out = _run_pixel(d, shape, weights, w_smooth, 0, prm)
    assert float(out.terms[1]) == 0.0 and _zero(out.g_illu), "constant illumination"
    xs, ys = W // 2 + 1, H // 3
    illu = torch.full((B, CI, H, W), 0.3)
    illu[:, 0, :, xs:] = 0.7
    if CI > 1:
        illu[:, CI - 1, ys:, :] = 0.55
    d["illu"] = illu
    out = _run_pixel(d, shape, weights, w_smooth, 0, prm)
    r64, r32 = (O.pixel_terms(d["low"], d["enh"], illu, d["refl"], weights, dict(prm, patch=patch), w_smooth, 0, dt)
                for dt in (torch.float64, torch.float32))
    want = torch.zeros((B, CI, H, W), dtype=torch.bool)
    want[:, 0, :, xs - 1:xs + 1] = True
    if CI > 1:
        want[:, CI - 1, ys - 1:ys + 1, :] = True
    assert np.array_equal(r64[3] != 0, want.numpy()), "the reference's own gradient support"
    assert torch.equal(out.g_illu != 0, want), "g_illu is non-zero exactly along the steps"
    _within_restated(f"g_illu steps | {shape}", out.g_illu, r64[3], _tt(r32[3]))
    _within_restated(f"term smoothness | steps {shape}", out.terms[1], r64[0][1], _tt(r32[0][1]))


def test_loss_workspace_sizes():
    """upr_t_loss_workspace is the _p form at patch 16; sizes are positive,
    grow with every dimension, and are 0 for arguments the entry refuses."""
    _, lib, _ = _lib()
    for B, H, W in ((1, 16, 16), (2, 64, 80), (3, 512, 512)):
        assert lib.upr_t_loss_workspace(B, H, W) == lib.upr_t_loss_workspace_p(B, H, W, 16) > 0
    base = lib.upr_t_loss_workspace_p(2, 64, 64, 4)
    assert lib.upr_t_loss_workspace_p(40, 64, 64, 4) > base and lib.upr_t_loss_workspace_p(2, 640, 64, 4) > base
    assert lib.upr_t_loss_workspace_p(2, 64, 640, 4) > base and lib.upr_t_loss_workspace_p(2, 64, 64, 1) > base
    for B, H, W, patch in ((0, 16, 16, 16), (1, 16, 16, 0), (1, 16, 16, -4), (1, 8, 16, 16), (1, 16, 8, 16), (1, 1, 8, 1)):
        assert lib.upr_t_loss_workspace_p(B, H, W, patch) == 0


@pytest.mark.parametrize("texture", [0, 1])
@pytest.mark.parametrize("shape", [(2, 16, 16, 16, 1), (1, 32, 272, 16, 1)], ids=lambda s: "x".join(map(str, s)))
def test_loss_pixel_default_entry(shape, texture):
    """upr_t_loss_pixel = upr_t_loss_pixel_p at the reference defaults (patch
    16, one illumination channel, dynamic smooth weight): both against float64
    within the same bound."""
    d = K.check_pixel_inputs(*shape)
    weights, w_smooth = (10.0, 0.5, 1.0, 0.1), 1.0
    prm = dict(O.DEFAULT_PARAMS)
    ref = _pixel_ref(shape, weights, w_smooth, texture, tuple(sorted(prm.items())))
    a = _run_pixel(d, shape, weights, w_smooth, texture, prm, default_entry=True)
    b = _run_pixel(d, shape, weights, w_smooth, texture, prm)
    _check_pixel(a, ref, "default entry", f"upr_t_loss_pixel texture={texture} {shape}")
    _check_pixel(b, ref, "default entry", f"upr_t_loss_pixel_p defaults texture={texture} {shape}")


def test_loss_pixel_refusals():
    """Every refused call leaves terms and the gradients untouched:
    upr_t_loss_pixel with H % 16 (UPR_ERR_SHAPE); _p with patch <= 0 or H or W
    < patch (UPR_ERR_SHAPE), illu_channels = 2 (UPR_ERR_UNSUPPORTED), texture
    = 2, a null params, a null input, and grads with a null gradient pointer
    (UPR_ERR_ARG)."""
    L, lib, st = _lib()
    B, H, W = 1, 24, 32
    d = {k: torch.rand(B, c, H, W).to(DEV) for k, c in (("low", 3), ("enh", 3), ("illu", 1), ("refl", 3))}
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    assert lib.upr_t_loss_workspace_p(B, H, W, 1) <= ws.numel()
    out = [Framed((9,)), Framed((B, 3, H, W)), Framed((B, 1, H, W)), Framed((B, 3, H, W))]
    ptrs = [o.ptr for o in out]
    ins = [P(d[k]) for k in ("low", "enh", "illu", "refl")]
    w = (1.0, 1.0, 1.0, 1.0, 1.0)

    def prm(patch=8, ci=1):
        return L.UprLossParams(patch, 0.6, 10.0, 1.0, 0.1, 1.0, 0.5, 1, ci)

    def call(ins=ins, H=H, W=W, ptrs=ptrs, grads=1, texture=0, cp=prm()):
        return lib.upr_t_loss_pixel_p(*ins, B, H, W, P(ws), *ptrs, grads, *w, texture,
                                      None if cp is None else ctypes.byref(cp), st)

    assert lib.upr_t_loss_pixel(*ins, B, H, W, P(ws), *ptrs, 1, *w, 0, st) == L.UPR_ERR_SHAPE  # 24 % 16
    assert lib.upr_t_loss_pixel(*ins, B, W, H, P(ws), *ptrs, 1, *w, 0, st) == L.UPR_ERR_SHAPE  # W % 16
    assert call(cp=prm(patch=0)) == L.UPR_ERR_SHAPE
    assert call(cp=prm(patch=-8)) == L.UPR_ERR_SHAPE
    assert call(cp=prm(patch=32)) == L.UPR_ERR_SHAPE   # H < patch
    assert call(H=W, W=H, cp=prm(patch=32)) == L.UPR_ERR_SHAPE   # W < patch
    assert call(cp=prm(ci=2)) == L.UPR_ERR_UNSUPPORTED
    assert call(texture=2) == L.UPR_ERR_ARG
    assert call(texture=-1) == L.UPR_ERR_ARG
    assert call(cp=None) == L.UPR_ERR_ARG
    for k in range(4):
        assert call(ins=ins[:k] + [None] + ins[k + 1:]) == L.UPR_ERR_ARG
    assert call(ptrs=[None] + ptrs[1:]) == L.UPR_ERR_ARG
    for k in (1, 2, 3):
        assert call(ptrs=ptrs[:k] + [None] + ptrs[k + 1:]) == L.UPR_ERR_ARG
    torch.cuda.synchronize()
    assert all(o.untouched() for o in out), "a refused call wrote an output"
    # grads = 0 takes null gradient pointers and writes the terms alone
    assert call(ptrs=[ptrs[0], None, None, None], grads=0) == 0
    torch.cuda.synchronize()
    t = out[0].get()
    assert bool((t[:5] != SENT).all()) and t[8] != SENT and all(o.untouched() for o in out[1:])


# ---------------------------------------------------------------------------
# texture complexity on its own
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,W", K.TEXTURE_CASES)
def test_texture_complexity(C, H, W):
    """upr_t_texture_complexity at B = 2: 'tv' against float64; the
    'edge_density' share bit-equal to float32(count / HW) of the float64
    reference (no magnitude is within 1e-5 of the threshold; on 2 x 2 every
    magnitude is exactly 0 and nothing is counted).  acc is scratch the entry
    zeroes itself."""
    _, lib, st = _lib()
    img = K.texture_inputs(C, H, W)
    K.check_edge_margin(img.numpy())
    B = img.shape[0]
    x = img.to(DEV)
    for method in (0, 1):
        acc = Framed((2 * B,), torch.float64, fill=777.25)
        out = Framed((B,))
        assert lib.upr_t_texture_complexity(P(x), B, C, H, W, method, acc.ptr, out.ptr, st) == 0
        torch.cuda.synchronize()
        acc.get("acc")
        got = out.get("out")
        ref = O.texture_complexity(img.numpy(), method)
        if method == 0:
            _within_restated(f"texture tv | C{C} {H}x{W}", got, ref, T.texture_complexity(img, "tv"))
        else:
            assert np.array_equal(got.numpy(), ref.astype(np.float32)), (got.tolist(), ref.tolist())
            print(f"BNOPS eq texture edge_density C{C} {H}x{W}: {got.tolist()}")
    assert torch.equal(x.cpu(), img)


def test_texture_complexity_refusals():
    L, lib, st = _lib()
    x = torch.rand(2, 3, 8, 8).to(DEV)
    acc, out = Framed((4,), torch.float64), Framed((2,))
    for B, C, H, W, method in ((0, 3, 8, 8, 0), (2, 0, 8, 8, 0), (2, 3, 8, 8, 2), (2, 3, 8, 8, -1)):
        assert lib.upr_t_texture_complexity(P(x), B, C, H, W, method, acc.ptr, out.ptr, st) == L.UPR_ERR_ARG
    for H, W in ((1, 8), (8, 1)):
        assert lib.upr_t_texture_complexity(P(x), 2, 3, H, W, 1, acc.ptr, out.ptr, st) == L.UPR_ERR_SHAPE
    assert lib.upr_t_texture_complexity(None, 2, 3, 8, 8, 0, acc.ptr, out.ptr, st) == L.UPR_ERR_ARG
    torch.cuda.synchronize()
    assert acc.untouched() and out.untouched()


# ---------------------------------------------------------------------------
# frequency
# ---------------------------------------------------------------------------
def _freq32(ze, zl, H, W, scale, w_high, w_low):
    """freq_kernel's formula in fp32 torch ops."""
    w = torch.where(torch.from_numpy(O.freq_low_mask(H, W)), torch.tensor(w_low), torch.tensor(w_high))[None]
    me = torch.sqrt(ze[..., 0] * ze[..., 0] + ze[..., 1] * ze[..., 1])
    ml = torch.sqrt(zl[..., 0] * zl[..., 0] + zl[..., 1] * zl[..., 1])
    dd = me - ml
    k = torch.where(me > 0, torch.tensor(scale) * 2.0 * w * dd / me, torch.zeros(()))
    return (w * dd * dd).sum(), k[..., None] * ze


def _cplx(z):
    return torch.view_as_complex(z.double()).numpy()


@pytest.mark.parametrize("H,W", K.FREQ_SHAPES)
def test_freq(H, W):
    """upr_t_freq_p with w_high != w_low (lattice points on the circle take
    w_low), some Ze exactly 0 (G = 0 there), into a non-zero acc[0] whose
    neighbours keep their sentinel; the G = NULL path; upr_t_freq = _p(1, 0.5)."""
    _, lib, st = _lib()
    if (H, W) == (20, 20):
        assert K.check_freq_lattice(H, W) == 12
    ze, zl = K.freq_inputs(H, W)
    BC, scale, pre = K.FREQ_BC, 0.37, 2.5
    w_high, w_low = K.FREQ_W
    zed, zld = ze.to(DEV), zl.to(DEV)
    s64, G64 = O.freq(_cplx(ze), _cplx(zl), H, W, scale, w_high, w_low)
    s32, G32 = _freq32(ze, zl, H, W, scale, w_high, w_low)
    G64 = np.stack([G64.real, G64.imag], -1)
    for with_g in (1, 0):
        acc = Framed((1,), torch.float64).set(torch.tensor([pre], dtype=torch.float64))
        G = Framed((BC, H, W, 2))
        assert lib.upr_t_freq_p(P(zed), P(zld), BC, H, W, acc.ptr, G.ptr if with_g else None, scale, w_high, w_low,
                                st) == 0
        torch.cuda.synchronize()
        _within_restated(f"freq sum | {H}x{W} G={with_g}", acc.get("acc")[0] - pre, np.float64(s64), s32)
        if with_g:
            g = G.get("G")
            _within_restated(f"freq G | {H}x{W}", g, G64, G32)
            zero = (ze == 0).all(-1)
            assert int(zero.sum()) == 3 and _zero(g[zero]), "G where |Ze| = 0"
        else:
            assert G.untouched()
    # the default entry: weights 1 / 0.5
    outs = []
    for entry in ("freq", "freq_p"):
        acc, G = Framed((1,), torch.float64, fill=0.0), Framed((BC, H, W, 2))
        if entry == "freq":
            rc = lib.upr_t_freq(P(zed), P(zld), BC, H, W, acc.ptr, G.ptr, scale, st)
        else:
            rc = lib.upr_t_freq_p(P(zed), P(zld), BC, H, W, acc.ptr, G.ptr, scale, 1.0, 0.5, st)
        torch.cuda.synchronize()
        assert rc == 0
        outs.append((acc.buf.cpu()[PAD], G.get("G")))
    s64, _ = O.freq(_cplx(ze), _cplx(zl), H, W, scale, 1.0, 0.5)
    s32, _ = _freq32(ze, zl, H, W, scale, 1.0, 0.5)
    assert torch.equal(outs[0][1], outs[1][1]), "upr_t_freq's G vs upr_t_freq_p(1, 0.5)"
    for (s, _), entry in zip(outs, ("upr_t_freq", "upr_t_freq_p(1, 0.5)")):
        _within_restated(f"freq sum | {H}x{W} {entry}", s, np.float64(s64), s32)
    assert torch.equal(zed.cpu(), ze) and torch.equal(zld.cpu(), zl)


def test_freq_refusals():
    L, lib, st = _lib()
    z = torch.randn(1, 4, 4, 2).to(DEV)
    acc, G = Framed((1,), torch.float64), Framed((1, 4, 4, 2))
    for a, b, c in ((None, P(z), acc.ptr), (P(z), None, acc.ptr), (P(z), P(z), None)):
        assert lib.upr_t_freq_p(a, b, 1, 4, 4, c, G.ptr, 1.0, 1.0, 0.5, st) == L.UPR_ERR_ARG
        assert lib.upr_t_freq(a, b, 1, 4, 4, c, G.ptr, 1.0, st) == L.UPR_ERR_ARG
    torch.cuda.synchronize()
    assert acc.untouched() and G.untouched()


# ---------------------------------------------------------------------------
# MSE
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("with_g", [1, 0])
@pytest.mark.parametrize("n", [1, 255, 4097, 2 ** 20 + 3])
def test_mse(n, with_g):
    """upr_t_mse: acc += mean (a - b)^2 into a non-zero acc, g = scale 2 (a -
    b) or G = NULL.  n = 2^20 + 3 is past the 4096-block cap: the stride loop."""
    _, lib, st = _lib()
    gen = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    scale, pre = float(np.float32(0.37 / n)), 1.5
    v64, g64 = O.mse(a.numpy(), b.numpy(), scale)
    acc = Framed((1,), torch.float64).set(torch.tensor([pre], dtype=torch.float64))
    g = Framed((n,))
    assert lib.upr_t_mse(P(a.to(DEV)), P(b.to(DEV)), n, acc.ptr, g.ptr if with_g else None, scale, st) == 0
    torch.cuda.synchronize()
    _within_restated(f"mse value | n{n} g={with_g}", acc.get("acc")[0] - pre, np.float64(v64), ((a - b) ** 2).mean())
    if with_g:
        _within_restated(f"mse g | n{n}", g.get("g"), g64, torch.tensor(scale) * 2.0 * (a - b))
    else:
        assert g.untouched()


@pytest.mark.parametrize("with_g", [1, 0])
@pytest.mark.parametrize("n", [4, 252, 4100, 2 ** 20 + 4])
def test_mse16(n, with_g):
    """upr_t_mse16 on fp16 inputs against float64 of the same fp16 values."""
    _, lib, st = _lib()
    gen = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=gen).half(), torch.randn(n, generator=gen).half()
    scale, pre = float(np.float32(0.37 / n)), 1.5
    v64, g64 = O.mse(a.double().numpy(), b.double().numpy(), scale)
    acc = Framed((1,), torch.float64).set(torch.tensor([pre], dtype=torch.float64))
    g = Framed((n,))
    assert lib.upr_t_mse16(P(a.to(DEV)), P(b.to(DEV)), n, acc.ptr, g.ptr if with_g else None, scale, st) == 0
    torch.cuda.synchronize()
    d32 = a.float() - b.float()
    _within_restated(f"mse16 value | n{n} g={with_g}", acc.get("acc")[0] - pre, np.float64(v64), (d32 ** 2).mean())
    if with_g:
        _within_restated(f"mse16 g | n{n}", g.get("g"), g64, torch.tensor(scale) * 2.0 * d32)
    else:
        assert g.untouched()


def test_mse_refusals_and_empty():
    """n == 0: UPR_OK from both entries with acc and g untouched (a mean of
    nothing must not put 0 / 0 into the accumulator).  upr_t_mse16 refuses n %
    4 != 0, a16 / b16 off 8-byte alignment and g off 16-byte alignment
    (UPR_ERR_UNSUPPORTED); null a, b or acc is UPR_ERR_ARG."""
    L, lib, st = _lib()
    a32, a16 = torch.randn(64).to(DEV), torch.randn(72).half().to(DEV)
    acc = Framed((1,), torch.float64).set(torch.tensor([1.5], dtype=torch.float64))
    g = Framed((64,))
    assert lib.upr_t_mse(P(a32), P(a32), 0, acc.ptr, g.ptr, 1.0, st) == L.UPR_OK
    assert lib.upr_t_mse16(P(a16), P(a16), 0, acc.ptr, g.ptr, 1.0, st) == L.UPR_OK
    assert P(a16) % 8 == 0 and P(a16, 1) % 8 == 2 and g.ptr % 16 == 0
    assert lib.upr_t_mse16(P(a16), P(a16), 62, acc.ptr, g.ptr, 1.0, st) == L.UPR_ERR_UNSUPPORTED
    assert lib.upr_t_mse16(P(a16, 1), P(a16), 64, acc.ptr, g.ptr, 1.0, st) == L.UPR_ERR_UNSUPPORTED
    assert lib.upr_t_mse16(P(a16), P(a16, 1), 64, acc.ptr, g.ptr, 1.0, st) == L.UPR_ERR_UNSUPPORTED
    assert lib.upr_t_mse16(P(a16), P(a16), 64, acc.ptr, g.ptr + 4, 1.0, st) == L.UPR_ERR_UNSUPPORTED
    for fn, x in ((lib.upr_t_mse, a32), (lib.upr_t_mse16, a16)):
        assert fn(None, P(x), 64, acc.ptr, g.ptr, 1.0, st) == L.UPR_ERR_ARG
        assert fn(P(x), None, 64, acc.ptr, g.ptr, 1.0, st) == L.UPR_ERR_ARG
        assert fn(P(x), P(x), 64, None, g.ptr, 1.0, st) == L.UPR_ERR_ARG
    torch.cuda.synchronize()
    assert float(acc.get()[0]) == 1.5 and g.untouched()


# ---------------------------------------------------------------------------
# VGG normalisation and the scalar helpers
# ---------------------------------------------------------------------------
def _bit_equal_share(dev, ref64):
    return float((dev.numpy() == np.asarray(ref64).astype(np.float32)).mean())


@pytest.mark.parametrize("B,H,W", [(2, 5, 7), (2, 33, 31)])
def test_vgg_norm(B, H, W):
    """upr_t_vgg_norm (NCHW -> NHWC) and upr_t_vgg_norm_bwd (adds into a
    non-zero NCHW g_x) within 1 ulp of float64 at B = 2 and odd H W (a wrong
    batch or plane stride shows).  g_x's start and g_y share a sign within a
    batch (+ in batch 0, - in batch 1).  Measured: neither is bit-equal
    throughout: 97% of the forward's and 78% of the backward's elements are
    (two roundings against the reference's one), the rest 1 ulp off."""
    _, lib, st = _lib()
    gen = torch.Generator().manual_seed(H * W)
    x = torch.rand(B, 3, H, W, generator=gen)
    sign = torch.tensor([1.0, -1.0]).view(2, 1, 1, 1)
    gy = sign * (torch.rand(B, H, W, 3, generator=gen) + 0.1)
    gx0 = sign * (torch.rand(B, 3, H, W, generator=gen) + 0.1)
    y = Framed((B, H, W, 3))
    assert lib.upr_t_vgg_norm(P(x.to(DEV)), y.ptr, B, H, W, st) == 0
    gx = Framed((B, 3, H, W)).set(gx0)
    assert lib.upr_t_vgg_norm_bwd(P(gy.to(DEV)), gx.ptr, B, H, W, st) == 0
    torch.cuda.synchronize()
    yr, gr = O.vgg_norm(x.numpy()), O.vgg_norm_bwd(gy.numpy(), gx0.numpy())
    print(f"BNOPS eq vgg_norm {B}x{H}x{W}: forward {_bit_equal_share(y.get(), yr):.4f} "
          f"backward {_bit_equal_share(gx.get(), gr):.4f} bit-equal")
    _within_ulp(f"vgg_norm {B}x{H}x{W}", y.get("y"), yr, ulps=1.0)
    _within_ulp(f"vgg_norm_bwd {B}x{H}x{W}", gx.get("g_x"), gr, ulps=1.0)


@pytest.mark.parametrize("n", [1, 1000])
def test_add_real(n):
    """upr_t_add_real: g += scale Re(z) within 1 ulp (the multiply-add may
    contract); Im(z) is not read into the result; g's start and Re(z) share a
    sign."""
    _, lib, st = _lib()
    gen = torch.Generator().manual_seed(n)
    z = torch.randn(n, 2, generator=gen)
    g0 = torch.sign(z[:, 0]) * (torch.rand(n, generator=gen) + 0.1)
    g = Framed((n,)).set(g0)
    assert lib.upr_t_add_real(P(z.to(DEV)), g.ptr, n, 0.3, st) == 0
    torch.cuda.synchronize()
    _within_ulp(f"add_real n{n}", g.get("g"), O.add_real(_cplx(z), g0.numpy(), 0.3), ulps=1.0)


def test_scale_acc():
    """upr_t_scale_acc: out[i] = float(acc[i] * scale) (a double product,
    rounded once) for n = 1, 3, 256, nothing past out[n - 1]; n = 0 and n =
    257 are UPR_ERR_ARG."""
    L, lib, st = _lib()
    acc = (torch.randn(300, dtype=torch.float64, generator=torch.Generator().manual_seed(9)) * 100).to(DEV)
    for n in (1, 3, 256):
        for scale in (1.0, 1.0 / 3):
            out = Framed((n,))
            assert lib.upr_t_scale_acc(P(acc), n, scale, out.ptr, st) == 0
            torch.cuda.synchronize()
            want = O.scale_acc(acc[:n].cpu().numpy(), scale).astype(np.float32)
            assert np.array_equal(out.get("out").numpy(), want)
    out = Framed((300,))
    for n in (0, 257, -1):
        assert lib.upr_t_scale_acc(P(acc), n, 1.0, out.ptr, st) == L.UPR_ERR_ARG
    assert lib.upr_t_scale_acc(None, 1, 1.0, out.ptr, st) == L.UPR_ERR_ARG
    assert lib.upr_t_scale_acc(P(acc), 1, 1.0, None, st) == L.UPR_ERR_ARG
    torch.cuda.synchronize()
    assert out.untouched()


def test_loss_total():
    """upr_t_loss_total: terms[7] within 2 ulp of the float64 weighted sum
    (terms[8] weighs the smoothness), the eight other slots bit-unchanged;
    w_freq = 0 drops the frequency term."""
    L, lib, st = _lib()
    t0 = torch.tensor([0.11, 0.034, 0.0071, 0.019, 0.0023, 1.37, 0.82, SENT, 0.787])
    for w in ((10.0, 0.5, 1.0, 0.1, 1.0, 0.5), (10.0, 0.5, 1.0, 0.1, 1.0, 0.0), (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)):
        t = Framed((9,)).set(t0)
        assert lib.upr_t_loss_total(t.ptr, *w, st) == 0
        torch.cuda.synchronize()
        got = t.get("terms")
        keep = [0, 1, 2, 3, 4, 5, 6, 8]
        assert torch.equal(got[keep], t0[keep]), "upr_t_loss_total wrote a slot other than [7]"
        _within_ulp(f"loss_total w_freq={w[5]}", got[7], O.loss_total(t0.numpy(), *w), ulps=2.0)
    with_f, without = O.loss_total(t0.numpy(), 10.0, 0.5, 1.0, 0.1, 1.0, 0.5), O.loss_total(t0.numpy(), 10.0, 0.5, 1.0,
                                                                                           0.1, 1.0, 0.0)
    assert with_f - without == pytest.approx(0.5 * float(t0[6]), rel=1e-6)
    assert lib.upr_t_loss_total(None, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, st) == L.UPR_ERR_ARG


# ---------------------------------------------------------------------------
# squared norm
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, 2 ** 19 + 5])
def test_sqsum(n):
    """upr_t_sqsum as a double against the float64 sum to 1e-12 (the products
    are formed in double: only the order of additions differs), from 0 and
    added to a non-zero acc (zeroing is the caller's job).  Values span 1e-4
    .. 1e2; n = 2^19 + 5 is past the 2048-block cap: the stride loop."""
    L, lib, st = _lib()
    gen = torch.Generator().manual_seed(n)
    g = torch.sign(torch.randn(n, generator=gen)) * 10 ** (torch.rand(n, generator=gen) * 6 - 4)
    gd = g.to(DEV)
    for pre in (0.0, 3.25):
        acc = Framed((1,), torch.float64).set(torch.tensor([pre], dtype=torch.float64))
        assert lib.upr_t_sqsum(P(gd), n, acc.ptr, st) == 0
        torch.cuda.synchronize()
        got, want = float(acc.get("acc")[0]), O.sqsum(g.numpy(), pre)
        print(f"BNOPS rel sqsum n{n} pre={pre}: {abs(got - want) / want:.3e}")
        assert abs(got - want) <= 1e-12 * want, (got, want)
    assert lib.upr_t_sqsum(None, n, acc.ptr, st) == L.UPR_ERR_ARG and lib.upr_t_sqsum(P(gd), n, None, st) == L.UPR_ERR_ARG
    assert torch.equal(gd.cpu(), g)
