"""Image-quality metrics and small helpers (reference utils/utils.py:95-333, :360-404).

The metric functions keep the reference's names, signatures and dict, and run
on the ROCm device: one launch pair of libupr.so (upr.runtime.image_metrics)
reads each image once and forms every metric in fp64; calculate_metrics then
makes one device-to-host copy.  Inputs are device tensors [3,H,W] / [1,3,H,W]
or numpy arrays in the reference's [H,W,C] layout (uploaded to the current
device); CPU tensors are refused like everywhere else in this package.
batch_metrics is the batched, non-synchronising form the reference lacks.
batch_loe / calculate_loe (an addition) give the lightness order error of an
enhanced image against its own low-light input (upr.runtime.image_loe);
batch_noise_sigma / calculate_noise_sigma (an addition) the blind noise level
of an image in u8 levels (upr.denoise.estimate_sigma on its to_u8_hwc pixels).

Divergences: the simplified NIQE clamps a window's variance at 0 (the
reference's float32 expression yields NaN on flat windows), and a batch is
measured image by image (the reference squeezes a batch of one).  The
reference's plotting helpers (visualize_results, plot_training_curves,
create_gif) are host-side matplotlib / PIL code and are not provided.
"""
import os

import numpy as np
import torch

from upr import _lib as L
from upr import runtime

# the reference dict's insertion order (utils.py:106-183); the three paired
# keys are present only with a reference image
_UNPAIRED = ("mean_brightness", "contrast", "entropy", "niqe", "saturation", "naturalness")
_PAIRED = ("mean_brightness", "contrast", "entropy", "niqe", "psnr", "ssim", "mse", "saturation", "naturalness")
_INDEX = {n: i for i, n in enumerate(L.METRIC_NAMES)}


def metric_names(paired):
    """Keys of calculate_metrics' dict, in its order."""
    return _PAIRED if paired else _UNPAIRED


def _as_batch(img, name):
    """[3,H,W] / [B,3,H,W] device tensor, or [H,W,3] / [3,H,W] / [1,3,H,W] numpy array -> [B,3,H,W] on the device."""
    if isinstance(img, np.ndarray):
        a = img
        if a.ndim == 4:
            a = a[0] if a.shape[0] == 1 else a
        if a.ndim == 3 and a.shape[0] != 3:  # the reference's test: [H,W,C] unless the first axis is 3
            a = a.transpose(2, 0, 1)
        if not torch.cuda.is_available():
            raise RuntimeError(
                f"{name} is a host array and no ROCm device is present: the UP-Retinex framework executes on "
                f"ROCm devices only (MI355X HIP kernels)")
        img = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.device("cuda",
                                                                                         torch.cuda.current_device()))
    runtime._require_device(img, name)
    if img.dim() == 3:
        img = img.unsqueeze(0)
    if img.dim() != 4 or img.shape[1] != 3:
        raise RuntimeError(f"{name}: expected an image of shape [3, H, W] or [B, 3, H, W], got {tuple(img.shape)}")
    if img.dtype not in (torch.float32, torch.float16):
        img = img.float()
    return img.detach()


def batch_metrics(enh, ref=None):
    """Every metric for every image of enh [B,3,H,W] (ref: same shape, optional):
    dict name -> float64 device tensor [B], in calculate_metrics' key order.  No
    synchronisation, no host copy."""
    x = _as_batch(enh, "img_enhanced")
    y = None
    if ref is not None:
        y = _as_batch(ref, "img_reference")
        if y.dtype != x.dtype:
            y = y.to(x.dtype)
    m, _, _ = runtime.image_metrics(x, y)
    return {n: m[:, _INDEX[n]] for n in metric_names(y is not None)}


def _single(enh, ref=None):
    x = _as_batch(enh, "img_enhanced")
    if x.shape[0] != 1:
        raise RuntimeError(f"expected one image, got a batch of {x.shape[0]} (use batch_metrics)")
    y = None
    if ref is not None:
        y = _as_batch(ref, "img_reference")
        if y.dtype != x.dtype:
            y = y.to(x.dtype)
    m, _, _ = runtime.image_metrics(x, y)
    return m[0].cpu().tolist(), y is not None  # the one device-to-host copy


def calculate_metrics(img_enhanced, img_reference=None):
    """The reference's dict of Python floats (utils.py:95-183)."""
    v, paired = _single(img_enhanced, img_reference)
    return {n: float(v[_INDEX[n]]) for n in metric_names(paired)}


def calculate_psnr(img1, img2):
    """PSNR in dB against a peak of 1.0; 100.0 when the MSE is below 1e-10 (utils.py:186-202)."""
    return float(_single(img1, img2)[0][_INDEX["psnr"]])


def calculate_ssim(img1, img2):
    """Mean over channels of the 11x11 box-window SSIM map (utils.py:205-247)."""
    return float(_single(img1, img2)[0][_INDEX["ssim"]])


def calculate_niqe(img):
    """The reference's simplified NIQE: mean local sigma over the spread of local means (utils.py:250-278)."""
    return float(_single(img)[0][_INDEX["niqe"]])


def calculate_saturation(img):
    """Mean of (max - min) / max over the pixels (utils.py:281-303)."""
    return float(_single(img)[0][_INDEX["saturation"]])


def calculate_naturalness(img):
    """0.3 colour balance + 0.4 contrast score + 0.3 brightness score (utils.py:306-333)."""
    return float(_single(img)[0][_INDEX["naturalness"]])


def batch_loe(img_low, img_enhanced, size=50):
    """Lightness order error (Wang et al. 2013, "Naturalness preserved
    enhancement algorithm for non-uniform illumination images") of every image
    of img_enhanced [B,3,H,W] against its low-light input img_low, on a
    size-pixel sample grid (0: every pixel): float64 device tensor [B].  No
    ground truth involved; no synchronisation, no host copy."""
    x = _as_batch(img_low, "img_low")
    y = _as_batch(img_enhanced, "img_enhanced")
    if y.dtype != x.dtype:
        y = y.to(x.dtype)
    return runtime.image_loe(x, y, size)


def calculate_loe(img_low, img_enhanced, size=50):
    """batch_loe of one image pair as a Python float (inputs as calculate_metrics takes them)."""
    v = batch_loe(img_low, img_enhanced, size)
    if v.shape[0] != 1:
        raise RuntimeError(f"expected one image, got a batch of {v.shape[0]} (use batch_loe)")
    return float(v.cpu()[0])


def batch_noise_sigma(img):
    """The blind noise estimate of every image of img [B,3,H,W] in u8 levels (the median
    Laplacian-difference estimator of upr.denoise.estimate_sigma, on the pixels to_u8_hwc
    gives a float image): float64 device tensor [B].  No synchronisation, no host copy."""
    from upr import denoise
    x = _as_batch(img, "img")
    return denoise.estimate_sigma(runtime.panels_u8(x, x, None, None)[0])


def calculate_noise_sigma(img):
    """batch_noise_sigma of one image as a Python float (inputs as calculate_metrics takes them)."""
    v = batch_noise_sigma(img)
    if v.shape[0] != 1:
        raise RuntimeError(f"expected one image, got a batch of {v.shape[0]} (use batch_noise_sigma)")
    return float(v.cpu()[0])


def ensure_dir(directory):
    """Create `directory` when it is missing (utils.py:360-369)."""
    if not os.path.exists(directory):
        os.makedirs(directory)
        print(f"Created directory: {directory}")


def count_parameters(model):
    """(total, trainable) parameter counts of a module (utils.py:372-386)."""
    total = trainable = 0
    for p in model.parameters():
        total += p.numel()
        if p.requires_grad:
            trainable += p.numel()
    return total, trainable


def print_model_summary(model):
    """Parameter counts of a module, printed (utils.py:389-404)."""
    total, trainable = count_parameters(model)
    bar = "=" * 60
    print(bar)
    print("Model Summary")
    print(bar)
    print(f"Total parameters: {total:,}")
    print(f"Trainable parameters: {trainable:,}")
    print(f"Non-trainable parameters: {total - trainable:,}")
    print(bar)
