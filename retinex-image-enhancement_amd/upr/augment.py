"""Device augmentation of a training batch (csrc/augment.hip via upr_augment):
the flips, rot90 and photometric chain of the reference's
LowLightDataset.__getitem__ (datasets/dataset.py:101-183) for [B,3,H,W] in one
call.  A sample's draw is a plain dict (datasets.dataset.draw_params); `pack`
turns a batch of them into the C records, in pinned host memory so the upload
is asynchronous.
"""
import ctypes

import numpy as np
import torch

from upr import _lib as L

# include/upr_train.h UprAugParams
RECORD = np.dtype([("flags", "<u4"), ("gamma", "<f4"), ("contrast", "<f4"), ("brightness", "<f4"),
                   ("noise_level", "<f4"), ("saturation", "<f4"), ("shift", "<f4"), ("reserved", "<u4"),
                   ("sample_id", "<u8")])
assert RECORD.itemsize == ctypes.sizeof(L.UprAugParams) == 40

# stage name -> flag bit, in the chain's order
STAGES = (("gamma", L.UPR_AUG_GAMMA), ("contrast", L.UPR_AUG_CONTRAST), ("brightness", L.UPR_AUG_BRIGHTNESS),
          ("noise_level", L.UPR_AUG_NOISE), ("saturation", L.UPR_AUG_SATURATION), ("shift", L.UPR_AUG_SHIFT))


def flags_of(p):
    """The flag word of one draw_params dict (a stage is on when its value is not None)."""
    f = (L.UPR_AUG_HFLIP if p.get("hflip") else 0) | (L.UPR_AUG_VFLIP if p.get("vflip") else 0)
    f |= (int(p.get("k", 0)) & 3) << L.UPR_AUG_ROT_SHIFT
    for name, bit in STAGES:
        if p.get(name) is not None:
            f |= bit
    return f


def pack(params, sample_ids, pin=True):
    """[dict] + [int] -> a uint8 host tensor holding the B records (pinned when a device is present)."""
    n = len(params)
    host = torch.empty(n * RECORD.itemsize, dtype=torch.uint8,
                       pin_memory=bool(pin) and torch.cuda.is_available())
    rec = host.numpy().view(RECORD)
    rec[:] = 0
    for i, (p, sid) in enumerate(zip(params, sample_ids)):
        rec[i]["flags"] = flags_of(p)
        for name, _ in STAGES:
            if p.get(name) is not None:
                rec[i][name] = p[name]
        rec[i]["sample_id"] = int(sid) & 0xFFFFFFFFFFFFFFFF
    return host


def target_records(params, sample_ids, pin=True):
    """The records of a batch's ground truth: each sample's flips and rot90, no
    photometric stage (only the low-light input is degraded further)."""
    return pack([{"hflip": p.get("hflip"), "vflip": p.get("vflip"), "k": p.get("k", 0)} for p in params],
                sample_ids, pin=pin)


def out_shape(flags, H, W):
    return (W, H) if (flags >> L.UPR_AUG_ROT_SHIFT) & 1 else (H, W)


_WS = {}


def _workspace(dev, nbytes):
    """One buffer per (device, stream): calls on a stream are ordered, so they may share it."""
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _WS[key] = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=dev)
    return ws


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def augment(x, records, seed=0, noise=None, out=None):
    """x [B,3,H,W] fp32 on a ROCm device, records = pack(...) -> y [B,3,Ho,Wo].
    Stream-ordered: the records are uploaded asynchronously and nothing waits.
    noise ([B,3,Ho,Wo]) replaces the generator's normals.  A batch whose images
    would differ in output shape raises RuntimeError and leaves `out` untouched."""
    if x.device.type != "cuda":
        raise RuntimeError("augment runs on ROCm devices only (no CPU fallback)")
    if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
        raise ValueError("augment expects a [B, 3, H, W] float32 tensor")
    B, _, H, W = x.shape
    rec = records.numpy().view(RECORD)
    if rec.shape[0] != B:
        raise ValueError(f"{rec.shape[0]} records for a batch of {B}")
    Ho, Wo = out_shape(int(rec[0]["flags"]), H, W)
    dev = x.device
    if not x.is_contiguous():
        x = x.contiguous()
    if out is None:
        out = torch.empty((B, 3, Ho, Wo), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (B, 3, Ho, Wo) or out.dtype != torch.float32 or not out.is_contiguous() \
            or out.device != dev:
        raise ValueError(f"out must be a contiguous float32 {(B, 3, Ho, Wo)} tensor on {dev}")
    if noise is not None:
        if tuple(noise.shape) != (B, 3, Ho, Wo) or noise.dtype != torch.float32 or noise.device != dev:
            raise ValueError(f"noise must be a float32 {(B, 3, Ho, Wo)} tensor on {dev}")
        noise = noise.contiguous()
    lib = L.lib()
    with torch.cuda.device(dev):
        ws = _workspace(dev, lib.upr_augment_workspace(B, H, W))
        rec_dev = records.to(dev, non_blocking=True)
        rc = lib.upr_augment(_ptr(x), _ptr(out), B, H, W, _ptr(rec_dev), _ptr(records), int(seed) & (2 ** 64 - 1),
                             _ptr(noise), _ptr(ws), ws.numel(), _stream(dev))
    L.check(rc, "upr_augment")
    return out


def normals(sample_ids, Ho, Wo, seed, device):
    """The generator alone (upr_augment_normals): [B,3,Ho,Wo] normals of the given sample ids."""
    dev = torch.device(device)
    records = pack([{} for _ in sample_ids], sample_ids)
    out = torch.empty((len(sample_ids), 3, Ho, Wo), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rec_dev = records.to(dev, non_blocking=True)
        rc = L.lib().upr_augment_normals(_ptr(out), len(sample_ids), Ho, Wo, _ptr(rec_dev),
                                         int(seed) & (2 ** 64 - 1), _stream(dev))
    L.check(rc, "upr_augment_normals")
    return out
