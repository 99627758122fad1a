"""Helpers shared by the op-level parity tests (test_gpu_bn_ops.py,
test_gpu_fam_ops.py): device pointers, channel slices of wider buffers with a
sentinel around them, and the two error bounds against a float64 reference
(ulp of the rounded reference; a multiple of the plain-fp32 restatement's own
error)."""
import numpy as np
import torch

DEV = "cuda"
SENT = -12345.5  # sentinel of channels / buffers a call must not write (exact in fp16 too)
# layout: (extra channels of the wider buffer, channel offset); off1 forces the unaligned fallback
LAYOUTS = {"contig": (0, 0), "slice4": (12, 4), "slice8": (12, 8), "off1": (3, 1)}


def P(t, off=0):
    return None if t is None else t.data_ptr() + off * t.element_size()


def _np(t):
    return t.detach().cpu().double().numpy()


def _wide(t, layout, fill=SENT):
    """t [M, C] placed as the channel slice of a [M, C + extra] device buffer
    otherwise holding `fill`; returns (buffer, channel stride, channel offset)."""
    extra, coff = LAYOUTS[layout]
    M, C = t.shape
    w = torch.full((M, C + extra), fill, dtype=t.dtype)
    w[:, coff:coff + C] = t
    return w.to(DEV), C + extra, coff


def _slice(w, coff, C):
    return w[:, coff:coff + C]


def _untouched(w, coff, C, what, fill=SENT):
    """Channels outside [coff, coff + C) still hold the sentinel, bit for bit."""
    for part in (w[:, :coff], w[:, coff + C:]):
        assert torch.equal(part, torch.full_like(part, fill)), f"{what}: wrote outside its channel slice"


def _ulp32(a):
    return np.spacing(np.abs(np.asarray(a, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def _within_ulp(what, dev, ref64, ulps=2.0, extra_rel=0.0):
    """|dev - float32(ref)| <= ulps * ulp(float32(ref)) (+ extra_rel * |ref|)."""
    dev = _np(dev)
    ref32 = np.asarray(ref64, dtype=np.float64).astype(np.float32).astype(np.float64)
    assert np.isfinite(dev).all(), what
    err = np.abs(dev - ref32)
    tol = ulps * _ulp32(ref32) + extra_rel * np.abs(ref32)
    print(f"BNOPS ulp {what}: max {np.max(err / _ulp32(ref32)):.2f} ulp, worst err/tol {np.max(err / tol):.3f}")
    assert (err <= tol).all(), f"{what}: {np.max(err / _ulp32(ref32)):.2f} ulp, err/tol {np.max(err / tol):.3f}"


def _within_restated(what, dev, ref64, restated, per_channel=False):
    """The kernel's error against the float64 reference is within 4x the error
    of the plain-fp32 restatement (at least half an ulp of the largest
    |reference|), per channel (axis 0 reduced) when asked; and under the
    op-level ceiling 1e-4 * max|ref| + 1e-6."""
    dev, rs, ref = _np(dev), _np(restated), np.asarray(ref64, dtype=np.float64)
    assert dev.shape == ref.shape == rs.shape, (what, dev.shape, ref.shape, rs.shape)
    assert np.isfinite(dev).all(), what
    e_dev, e_rs, a = np.abs(dev - ref), np.abs(rs - ref), np.abs(ref)
    if per_channel:
        e_dev, e_rs, a = e_dev.max(axis=0), e_rs.max(axis=0), a.max(axis=0)
    else:
        e_dev, e_rs, a = e_dev.max(), e_rs.max(), a.max()
    bound = 4.0 * np.maximum(e_rs, 0.5 * _ulp32(a))
    u = _ulp32(np.max(a))
    print(f"BNOPS rst {what}: restated {np.max(e_rs) / u:.2f} ulp kernel {np.max(e_dev) / u:.2f} ulp "
          f"(abs {np.max(e_rs):.3e} / {np.max(e_dev):.3e}) worst kernel/bound {np.max(e_dev / bound):.3f}")
    ceil = 1e-4 * np.max(a) + 1e-6
    assert np.max(e_dev) <= ceil, f"{what}: max|d| {np.max(e_dev):.3e} > ceiling {ceil:.3e}"
    assert (e_dev <= bound).all(), f"{what}: kernel error / bound {np.max(e_dev / bound):.3f}"
