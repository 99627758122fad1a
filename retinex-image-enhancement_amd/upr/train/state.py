"""The engine's switches: autocast, fp16-only stores, the cast trace, per-call conv timing."""
import os

import torch

# Autocast (AMP) arithmetic.  The reference runs the model forward and the
# loss under torch.cuda.amp.autocast() when use_amp (trainers/train.py:71-75),
# i.e. its convolutions in fp16.  The graph / loss engine set this flag from
# the caller's autocast state at forward time; while set, MFMA convs (and the
# input gradients of their backward) run on the fp16 kernels with fp32
# accumulation and fp32 activations in between (upr_t_conv_mfma16).  Weight
# gradients, BatchNorm, losses, FFTs and the optimiser stay fp32.
_AMP = [False]


# UPR_TRACE_CAST=1: name the convs whose fp16 operand is cast at the conv (conv.mfma16)
_TRACE_CAST = os.environ.get("UPR_TRACE_CAST", "0") == "1"
# fp16-only activation stores (the FAM / ASPP concats, FAM branch and pool
# outputs, scale stems) where no reader needs the fp32 value; False writes the
# fp32 values too (the gradients must not change: tests/test_gpu_train.py
# test_amp_fp16_only_stores_bitwise)
FP16_ONLY_STORES = [True]


def autocast_active():
    """True inside torch.autocast('cuda') (any half dtype: the kernels compute fp16)."""
    try:
        return bool(torch.is_autocast_enabled("cuda"))
    except TypeError:  # older signature
        return bool(torch.is_autocast_enabled())


def set_amp(on):
    _AMP[0] = bool(on)


# Per-call device timing of the conv launches (bench.py's training roofline).
# While profile_begin() is active every conv call below records a HIP event
# pair on the current stream around its library call(s), tagged with its
# arithmetic ("mfma16": fp16 MFMA with fp32 accumulation, "mfma32": fp32
# MFMA, "direct": FMA kernels) and its ALGORITHMIC flops 2*B*Ho*Wo*Cout*Cin*k^2
# (forward, input gradient and weight gradient each count one such product;
# the zero-upsampled stride-2 input gradient executes 4x that and is charged 1x).
_PROF = [None]


def profile_begin():
    _PROF[0] = []


def profile_end():
    """Stops recording; returns [(kind, what, flops, ms, shape)] (synchronises);
    shape: (Cin, Cout, k, stride, H, W) of the conv's input, or None."""
    recs, _PROF[0] = _PROF[0], None
    if not recs:
        return []
    torch.cuda.synchronize()
    return [(k, w, f, e0.elapsed_time(e1), sh) for k, w, f, e0, e1, sh in recs]


class _timed:
    __slots__ = ("rec",)

    def __init__(self, kind, what, flops, shape=None):
        self.rec = None
        if _PROF[0] is not None and kind is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.rec = [kind, what, flops, e0, e1, shape]

    def __enter__(self):
        if self.rec is not None:
            self.rec[3].record()
        return self

    def __exit__(self, *exc):
        if self.rec is not None:
            self.rec[4].record()
            _PROF[0].append(tuple(self.rec))
        return False

