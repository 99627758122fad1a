"""Enhance harness (drop-in for reference enhancers/simple_enhance.py).

Image decode stays on the host (PIL); everything between load and save runs on
the device.  PNG encode is the host's (PIL, the default) or, with
png_encoder="device", the device's (upr.png: larger files, no host encode);
png_encoder="device_lz" is the device's with LZ77 matching (smaller files).
image_format="jpg" (an addition; the default "png" changes nothing) writes the
three files as baseline JPEGs of quality jpeg_quality: PIL with the host encoder,
upr.jpeg (the device's own integer DCT) with either device encoder.  With either,
jpeg_subsampling="420" halves the chroma of all three files (the default "444" does
not), jpeg_optimize=True gives every file Huffman tables of its own and
jpeg_gray_maps=True writes _illumination.jpg as a one-component file (the enhanced
file and the comparison stay colour); image_format="png" ignores the three.
Intentional divergences, each a reference bug:
  * enhance_single_image accepts and ignores `adjuster=` so main.py's
    single-file branch works (reference main.py:240-249 vs simple_enhance.py:135
    raises TypeError);
  * enhance_batch_images takes optional use_preact/use_aspp/seed (defaults keep
    the reference behaviour: UP_Retinex() defaults, unseeded init).
output_size="original" (an addition; the default "letterbox" changes nothing) writes the three
files at the source's size: the letterboxed result is carried to the decoded image's pixels by
the guided-filter restore of upr.guided (radius guided_radius, regulariser guided_eps), or, when
the letterbox resized nothing, by cropping the bars away.
denoise="nlm" (an addition; the default "off" changes nothing) runs the illumination-weighted
non-local means of upr.denoise on the enhanced image's u8 pixels before they are written (after
CLAHE; inside the letterbox's content rectangle; strength denoise_strength * 255 / max(illumination,
denoise_floor) levels per pixel, search radius denoise_search, patch radius denoise_patch): the
_enhanced file and the comparison's enhanced panel hold the denoised pixels, the _illumination
file and the returned tensors do not change.  With output_size="original" the letterboxed pixels
are denoised and the guided restore carries them to the source's size.
denoise_strength="auto" measures every image's noise level instead (upr.denoise.estimate_sigma on
the input's u8 pixels, the comparison's left panel, inside the content rectangle) and filters it
with denoise_auto_scale times that estimate: per image, on the device, nothing comes to the host.
enhance_batch_images(batch_size > 1) and main.py --infer_batch run the batched
directory path (run_batched): files grouped by letterboxed shape (plan_batches),
one upload + upr_letterbox_batch, one forward, one CLAHE, one upr_panels_u8 and
three batched PNG encodes per batch, two batches in flight.
"""
import functools
import os
from typing import NamedTuple
from collections import deque
from concurrent.futures import ThreadPoolExecutor
import threading
import time

import numpy as np
import torch
from PIL import Image

from models.model import UP_Retinex
from enhancers.adaptive_params import AdaptiveParameterAdjuster
from enhancers.multi_scale import MultiScaleEnhancer
from enhancers.content_aware import ContentAwareEnhancer
from utils.letterbox import letterbox_content, letterbox_shape, letterbox_u8_batch, letterbox_u8_image

# Writer threads running beside the GPU; 3 files per image.
# png_encoder="host": each writer runs PIL's PNG encoder (it releases the GIL), ~90 /
# ~160 ms of host CPU for a 512^2 / comparison PNG of a noisy image, so the batch
# harness is encode-bound: one writer per usable core but two, at most 14
# (os.cpu_count() is the whole machine on a shared box; UPR_PNG_WRITERS overrides).
# png_encoder="device": the files are encoded on the GPU (upr.png) behind the image's
# other launches; a writer only waits for them, copies the file's bytes and writes them.
# png_encoder="device_lz": the same with upr.png's matches="lz".
PNG_ENCODERS = ("host", "device", "device_lz")
_DEVICE_MATCHES = {"device": "none", "device_lz": "lz"}


def _check_encoder(png_encoder):
    if png_encoder not in PNG_ENCODERS:
        raise ValueError(f"png_encoder must be one of {PNG_ENCODERS}, got {png_encoder!r}")


IMAGE_FORMATS = ("png", "jpg")


JPEG_SUBSAMPLINGS = ("444", "420")


def _check_format(image_format, jpeg_quality, jpeg_subsampling="444", jpeg_optimize=False, jpeg_gray_maps=False):
    if image_format not in IMAGE_FORMATS:
        raise ValueError(f"image_format must be one of {IMAGE_FORMATS}, got {image_format!r}")
    if image_format != "jpg":
        return
    if not 1 <= int(jpeg_quality) <= 100:
        raise ValueError(f"jpeg_quality must be in 1..100, got {jpeg_quality!r}")
    if jpeg_subsampling not in JPEG_SUBSAMPLINGS:
        raise ValueError(f"jpeg_subsampling must be one of {JPEG_SUBSAMPLINGS}, got {jpeg_subsampling!r}")
    for name, v in (("jpeg_optimize", jpeg_optimize), ("jpeg_gray_maps", jpeg_gray_maps)):
        if not isinstance(v, bool):
            raise ValueError(f"{name} must be True or False, got {v!r}")


class _Jpeg(NamedTuple):
    """How one .jpg file is written: what the public jpeg_* arguments mean for that file."""
    quality: int = 95
    subsampling: str = "444"
    optimize: bool = False
    gray: bool = False  # a one-component file (the illumination map with jpeg_gray_maps)

    def colour(self):
        return self._replace(gray=False)


OUTPUT_SIZES = ("letterbox", "original")


def _check_output_size(output_size, guided_radius, guided_eps):
    if output_size not in OUTPUT_SIZES:
        raise ValueError(f"output_size must be one of {OUTPUT_SIZES}, got {output_size!r}")
    from upr import guided
    guided.check_params(guided_radius, guided_eps)


DENOISERS = ("off", "nlm")


class _Denoise(NamedTuple):
    """The public denoise* arguments, checked."""
    mode: str = "off"
    strength: float = 1.0
    floor: int = 16
    search: int = 5
    patch: int = 2
    auto: bool = False       # denoise_strength="auto": every image's own estimate ...
    auto_scale: float = 1.0  # ... times this

    @property
    def on(self):
        return self.mode == "nlm"

    @property
    def public_strength(self):
        return "auto" if self.auto else self.strength

    def apply(self, enh_u8, illu_u8, content, low_u8):
        """u8 [B,H,W,3] enhanced / illumination / input pixels on the device -> the denoised enhanced
        pixels.  low_u8 is read with auto alone: three launches on the current stream, no host copy."""
        from upr import denoise
        if self.auto:
            return denoise.nlm_auto(enh_u8, low_u8, illu_u8, content, self.auto_scale, self.floor, self.search,
                                    self.patch)
        return denoise.nlm(enh_u8, illu_u8, content, self.strength, self.floor, self.search, self.patch)


def _check_denoise(denoise, denoise_strength=1.0, denoise_floor=16, denoise_search=5, denoise_patch=2,
                   denoise_auto_scale=1.0):
    if denoise not in DENOISERS:
        raise ValueError(f"denoise must be one of {DENOISERS}, got {denoise!r}")
    from upr import denoise as upr_denoise
    upr_denoise.check_params(denoise_strength, denoise_floor, denoise_search, denoise_patch, denoise_auto_scale)
    auto = isinstance(denoise_strength, str)
    return _Denoise(denoise, 1.0 if auto else float(denoise_strength), int(denoise_floor), int(denoise_search),
                    int(denoise_patch), auto, float(denoise_auto_scale))


def _writer_count():
    try:
        n = int(os.environ.get("UPR_PNG_WRITERS", "0"))
    except ValueError:
        n = 0
    return n if n > 0 else min(14, max(2, (os.cpu_count() or 8) - 2))


_WRITERS = _writer_count()
VALID_EXTENSIONS = {'.jpg', '.jpeg', '.png', '.bmp', '.tif', '.tiff'}


def _decode(image_path):
    """PIL decode -> (uint8 HWC RGB array, (W, H)).  Runs on the harness's
    prefetch thread for the next file of a batch."""
    img = Image.open(image_path).convert('RGB')
    return np.array(img, dtype=np.uint8), img.size


def load_image(image_path, max_size=None, device=None, decoded=None):
    """Decode + letterbox (reference :23-62) -> ([1,3,H,W] float32, (W, H)).

    The decoded uint8 pixels go to the ROCm device as bytes and ToTensor +
    letterbox_tensor run there as one launch (utils/letterbox.py); the tensor is
    returned on that device (the reference returns it on the CPU and the caller
    moves it -- the callers' .to(device) is then a no-op).  `decoded` takes an
    already decoded (array, size) pair (the batch harness's prefetch)."""
    a, original_size = decoded if decoded is not None else _decode(image_path)
    new_shape = max_size if max_size is not None else a.shape[:2]
    t, _, _ = letterbox_u8_image(a, new_shape=new_shape, auto=True, scaleup=False, device=device)
    return t.unsqueeze(0), original_size


def _to_u8_hwc(t):
    """(np.clip(x, 0, 1) * 255).astype(np.uint8) of one [C,H,W] image, 1-channel
    maps replicated to RGB (reference :65-99): one device launch, then the
    3 B/pixel copy to the host for the PNG encoder."""
    from upr import runtime
    return runtime.to_u8_hwc(t.detach()).cpu().numpy()


def _to_u8_hwc_device(t):
    """The same pixels as _to_u8_hwc, left on the device (png_encoder="device")."""
    from upr import runtime
    return runtime.to_u8_hwc(t.detach())


def _write_png(arr, save_path, msg):
    Image.fromarray(arr).save(save_path)
    print(f"{msg}: {save_path}")


def _write_jpg(arr, save_path, msg, jpeg):
    im = Image.fromarray(arr)
    if jpeg.gray:  # exact for the maps' R = G = B; one component has nothing to subsample
        im = im.convert("L")
    im.save(save_path, format="JPEG", quality=int(jpeg.quality), optimize=bool(jpeg.optimize),
            subsampling=2 if jpeg.subsampling == "420" and not jpeg.gray else 0)
    print(f"{msg}: {save_path}")


def _pixel_writer(image_format, jpeg):
    """The host encoder of a format: f(arr, save_path, msg)."""
    return _write_png if image_format == "png" else functools.partial(_write_jpg, jpeg=jpeg)


def _emit(arr, save_path, msg, writer, image_format="png", jpeg=_Jpeg()):
    write = _pixel_writer(image_format, jpeg)
    if writer is None:
        write(arr, save_path, msg)
    else:  # encode + file write on the batch harness's writer thread
        writer.submit(write, arr, save_path, msg)


def _write_device_pngs(buf, sizes, done, jobs):
    """Files of one upr.png / upr.jpeg encode_device call: wait for it, copy sizes[b] bytes of image b
    and write them (no encoding on the host)."""
    done.synchronize()
    for b, n in enumerate(sizes.tolist()):
        data = buf[b, :n].cpu().numpy().tobytes()
        save_path, msg = jobs[b]
        with open(save_path, "wb") as fh:
            fh.write(data)
        print(f"{msg}: {save_path}")


def _encode_device(u8_images, png_encoder, image_format, jpeg):
    """(buf, sizes) of the device encoder of a format; queued on the current stream."""
    if image_format == "jpg":
        from upr import jpeg as upr_jpeg
        return upr_jpeg.encode_device(u8_images, quality=jpeg.quality,
                                      subsampling="gray" if jpeg.gray else jpeg.subsampling, optimize=jpeg.optimize)
    from upr import png
    return png.encode_device(u8_images, matches=_DEVICE_MATCHES[png_encoder])


def _emit_device(u8_images, jobs, writer, png_encoder, image_format="png", jpeg=_Jpeg()):
    """u8_images: u8 [B,H,W,3] (or [H,W,3]) on the device, jobs: (save_path, msg) per image.
    The encode is queued on the current stream here; the copy and the write happen on the
    writer thread (or right away without one)."""
    buf, sizes = _encode_device(u8_images, png_encoder, image_format, jpeg)
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(buf.device))
    if writer is None:
        _write_device_pngs(buf, sizes, done, jobs)
    else:
        writer.submit(_write_device_pngs, buf, sizes, done, jobs)


def save_image(tensor, save_path, writer=None, png_encoder="host", image_format="png", jpeg_quality=95,
               jpeg_subsampling="444", jpeg_optimize=False, jpeg_gray_maps=False):
    """[1,C,H,W] or [C,H,W] -> PNG; 1-channel maps are replicated to RGB (reference :65-99).
    image_format="jpg": the same pixels as a JPEG of quality jpeg_quality, chroma as
    jpeg_subsampling says, Huffman tables of its own with jpeg_optimize; jpeg_gray_maps=True
    says the tensor is a map (the caller's _illumination file): a one-component file."""
    _check_encoder(png_encoder)
    _check_format(image_format, jpeg_quality, jpeg_subsampling, jpeg_optimize, jpeg_gray_maps)
    jpeg = _Jpeg(jpeg_quality, jpeg_subsampling, jpeg_optimize, jpeg_gray_maps)
    if tensor.dim() == 4:
        tensor = tensor.squeeze(0)
    if png_encoder in _DEVICE_MATCHES:
        _emit_device(_to_u8_hwc_device(tensor), [(save_path, "已保存")], writer, png_encoder, image_format, jpeg)
    else:
        _emit(_to_u8_hwc(tensor), save_path, "已保存", writer, image_format, jpeg)


def create_comparison(img_low, img_enhanced, save_path, writer=None, illu_map=None, png_encoder="host",
                      image_format="png", jpeg_quality=95, jpeg_subsampling="444", jpeg_optimize=False,
                      jpeg_gray_maps=False):
    """[input | enhanced] side by side (reference :102-132); with `illu_map`
    the predictor's 3-panel form [input | enhanced | illumination]
    (reference predictors/predict.py:102-140).  The comparison is a colour file whatever
    jpeg_gray_maps says."""
    _check_encoder(png_encoder)
    _check_format(image_format, jpeg_quality, jpeg_subsampling, jpeg_optimize, jpeg_gray_maps)
    jpeg = _Jpeg(jpeg_quality, jpeg_subsampling, jpeg_optimize)
    to_u8 = _to_u8_hwc_device if png_encoder in _DEVICE_MATCHES else _to_u8_hwc
    panels = [to_u8(img_low.squeeze(0)), to_u8(img_enhanced.squeeze(0))]
    if illu_map is not None:
        panels.append(to_u8(illu_map.squeeze(0)))
    if png_encoder in _DEVICE_MATCHES:  # the panel is joined on the device, along W
        _emit_device(torch.cat(panels, dim=1), [(save_path, "已保存对比图像")], writer, png_encoder,
                     image_format, jpeg)
    else:
        _emit(np.concatenate(panels, axis=1), save_path, "已保存对比图像", writer, image_format, jpeg)


def save_original_size(src_u8, img_low, img_enhanced, illu_map, paths, max_size=None, comparison=2, writer=None,
                       png_encoder="host", image_format="png", jpeg_quality=95, guided_radius=4, guided_eps=1e-4,
                       jpeg_subsampling="444", jpeg_optimize=False, jpeg_gray_maps=False, denoise="off",
                       denoise_strength=1.0, denoise_floor=16, denoise_search=5, denoise_patch=2,
                       denoise_auto_scale=1.0):
    """The three files of one image at the source's size (output_size="original").  src_u8: the
    decoded uint8 HWC image; img_low / img_enhanced / illu_map: the [1,C,H',W'] letterboxed
    tensors whose pixels the files hold with output_size="letterbox"; paths: (enhanced,
    illumination, comparison) file names, the last unused with comparison=None (2: [input |
    enhanced], 3: [input | enhanced | illumination]).  upr.guided.restore on those pixels;
    denoise="nlm" denoises the letterboxed enhanced pixels first (the restore's target)."""
    from upr import guided, runtime
    dn = _check_denoise(denoise, denoise_strength, denoise_floor, denoise_search, denoise_patch, denoise_auto_scale)
    H, W = src_u8.shape[:2]
    content = letterbox_content((H, W), max_size if max_size is not None else (H, W), auto=True, scaleup=False)
    dev = img_enhanced.device

    def u8(t):
        return runtime.to_u8_hwc(t.detach().squeeze(0).to(dev)).unsqueeze(0)

    src = torch.from_numpy(np.ascontiguousarray(src_u8)).to(dev).unsqueeze(0)
    low_u8, target, illu_u8 = u8(img_low), u8(img_enhanced), u8(illu_map)
    if dn.on:
        target = dn.apply(target, illu_u8, content, low_u8)
    outs = guided.restore(src, low_u8, target, illu_u8, content, guided_radius, guided_eps, comparison)
    colour = _Jpeg(jpeg_quality, jpeg_subsampling, jpeg_optimize)
    modes = (colour, colour._replace(gray=bool(jpeg_gray_maps)), colour)
    for arr, path, msg, jpeg in zip(outs, paths, ("已保存", "已保存", "已保存对比图像"), modes):
        if arr is None:
            continue
        if png_encoder in _DEVICE_MATCHES:
            _emit_device(arr[0], [(path, msg)], writer, png_encoder, image_format, jpeg)
        else:
            _emit(arr[0].cpu().numpy(), path, msg, writer, image_format, jpeg)


def save_denoised(img_low, img_enhanced, illu_map, paths, content, comparison=2, writer=None, png_encoder="host",
                  image_format="png", jpeg_quality=95, jpeg_subsampling="444", jpeg_optimize=False,
                  jpeg_gray_maps=False, denoise="nlm", denoise_strength=1.0, denoise_floor=16, denoise_search=5,
                  denoise_patch=2, denoise_auto_scale=1.0):
    """The three letterboxed files of one image with denoise="nlm": the pixels save_image and
    create_comparison write, the enhanced ones denoised inside the content rectangle `content`
    (utils.letterbox.letterbox_content) with the illumination file's pixels as the strength map.
    paths and comparison as in save_original_size."""
    from upr import runtime
    dn = _check_denoise(denoise, denoise_strength, denoise_floor, denoise_search, denoise_patch, denoise_auto_scale)
    dev = img_enhanced.device
    low, enh, illu = (runtime.to_u8_hwc(t.detach().squeeze(0).to(dev)) for t in (img_low, img_enhanced, illu_map))
    if dn.on:
        enh = dn.apply(enh.unsqueeze(0), illu.unsqueeze(0), content, low.unsqueeze(0))[0]
    cmp = torch.cat([low, enh] + ([illu] if comparison == 3 else []), dim=1) if comparison else None
    colour = _Jpeg(jpeg_quality, jpeg_subsampling, jpeg_optimize)
    modes = (colour, colour._replace(gray=bool(jpeg_gray_maps)), colour)
    for arr, path, msg, jpeg in zip((enh, illu, cmp), paths, ("已保存", "已保存", "已保存对比图像"), modes):
        if arr is None:
            continue
        if png_encoder in _DEVICE_MATCHES:
            _emit_device(arr, [(path, msg)], writer, png_encoder, image_format, jpeg)
        else:
            _emit(arr.cpu().numpy(), path, msg, writer, image_format, jpeg)


def enhance_single_image(model, image_path, output_dir, device, max_size=None, enable_multi_scale=False,
                         enable_content_aware=False, adjuster=None, precision="fp32", _decoded=None, _writer=None,
                         png_encoder="host", image_format="png", jpeg_quality=95, output_size="letterbox",
                         guided_radius=4, guided_eps=1e-4, jpeg_subsampling="444", jpeg_optimize=False,
                         jpeg_gray_maps=False, denoise="off", denoise_strength=1.0, denoise_floor=16, denoise_search=5,
                         denoise_patch=2, denoise_auto_scale=1.0):
    """Enhance one file and write {name}_enhanced/_illumination/_comparison.png (reference :135-199;
    .jpg with image_format="jpg", quality jpeg_quality; jpeg_subsampling and jpeg_optimize apply to
    all three files, jpeg_gray_maps makes _illumination.jpg a one-component file).
    precision="fp16" runs the fp16 storage / fp16-MFMA graph (input cast to half).
    png_encoder="device" encodes the three files on the GPU (same pixels, larger files),
    "device_lz" does so with LZ77 matching (same pixels, smaller files than "device").
    output_size="original" writes the three files at the source's size (save_original_size);
    the returned tensors stay the letterboxed ones.  denoise="nlm" writes the enhanced pixels
    denoised (upr.denoise.nlm, after CLAHE, whichever enhancer ran); the returned tensors are not.
    denoise_strength="auto": the strength is denoise_auto_scale times the input's measured noise level."""
    _check_encoder(png_encoder)
    _check_format(image_format, jpeg_quality, jpeg_subsampling, jpeg_optimize, jpeg_gray_maps)
    _check_output_size(output_size, guided_radius, guided_eps)
    dn = _check_denoise(denoise, denoise_strength, denoise_floor, denoise_search, denoise_patch, denoise_auto_scale)
    noise = dict(denoise=dn.mode, denoise_strength=dn.public_strength, denoise_floor=dn.floor,
                 denoise_search=dn.search, denoise_patch=dn.patch, denoise_auto_scale=dn.auto_scale)
    print(f"正在处理: {os.path.basename(image_path)}")
    if _decoded is None and (output_size == "original" or dn.on):
        _decoded = _decode(image_path)
    img_low, _ = load_image(image_path, max_size, decoded=_decoded)
    if precision == "fp16":
        img_low = img_low.half()
    adjuster = AdaptiveParameterAdjuster()
    multi_scale_enhancer = MultiScaleEnhancer()
    content_aware_enhancer = ContentAwareEnhancer()
    start = time.time()
    if enable_content_aware:
        img_enhanced, illu_map = content_aware_enhancer.apply_content_aware_enhancement(model, img_low, device)
    elif enable_multi_scale:
        img_enhanced, illu_map = multi_scale_enhancer.enhance_with_pyramid(model, img_low, device)
    else:
        img_enhanced, illu_map = adjuster.apply_adaptive_enhancement(model, img_low, device)
    if torch.cuda.is_available() and img_enhanced.is_cuda:
        torch.cuda.synchronize(img_enhanced.device)
    print(f"增强耗时: {time.time() - start:.4f}s")
    os.makedirs(output_dir, exist_ok=True)
    name = os.path.splitext(os.path.basename(image_path))[0]
    fmt = dict(image_format=image_format, jpeg_quality=jpeg_quality, jpeg_subsampling=jpeg_subsampling,
               jpeg_optimize=jpeg_optimize)
    if output_size == "original":
        save_original_size(_decoded[0], img_low, img_enhanced, illu_map,
                           [os.path.join(output_dir, f"{name}_{kind}.{image_format}")
                            for kind in ("enhanced", "illumination", "comparison")], max_size, 2, _writer,
                           png_encoder, guided_radius=guided_radius, guided_eps=guided_eps,
                           jpeg_gray_maps=jpeg_gray_maps, **fmt, **noise)
        print("图像增强完成！")
        return img_enhanced, illu_map
    if dn.on:
        shape = _decoded[0].shape[:2]
        save_denoised(img_low, img_enhanced, illu_map,
                      [os.path.join(output_dir, f"{name}_{kind}.{image_format}")
                       for kind in ("enhanced", "illumination", "comparison")],
                      letterbox_content(shape, max_size if max_size is not None else shape, auto=True, scaleup=False),
                      2, _writer, png_encoder, jpeg_gray_maps=jpeg_gray_maps, **fmt, **noise)
        print("图像增强完成！")
        return img_enhanced, illu_map
    save_image(img_enhanced, os.path.join(output_dir, f"{name}_enhanced.{image_format}"), _writer, png_encoder, **fmt)
    save_image(illu_map, os.path.join(output_dir, f"{name}_illumination.{image_format}"), _writer, png_encoder,
               jpeg_gray_maps=jpeg_gray_maps, **fmt)
    create_comparison(img_low, img_enhanced, os.path.join(output_dir, f"{name}_comparison.{image_format}"), _writer,
                      png_encoder=png_encoder, **fmt)
    print("图像增强完成！")
    return img_enhanced, illu_map


def list_images(input_dir):
    files = [os.path.join(input_dir, f) for f in os.listdir(input_dir)
             if os.path.splitext(f)[1].lower() in VALID_EXTENSIONS]
    return sorted(files)


# ---------------------------------------------------------------------------
# the batched directory path
# ---------------------------------------------------------------------------
MAX_OPEN_BUCKETS = 8
# CPUs the batched path plans for (a shared machine gives a command 16, whatever os.cpu_count()
# says): decode threads + writer threads stay within it; the 2 copier threads only wait for an
# event and for their copies
_BATCH_CPUS = 16
_COPIERS = 2


def plan_batches(shapes, batch_size):
    """Batches of file indices for the batched path: shapes[i] is the letterboxed (H, W) of
    file i in listing order -> list of index lists, each of one shape and at most batch_size
    long.  One bucket is open per shape; a bucket is emitted when it holds batch_size indices,
    the rest at the end in order of each bucket's first index.  At most MAX_OPEN_BUCKETS are
    open: a further shape first emits the bucket with the oldest first index, short.  Every
    index appears exactly once; pure and deterministic."""
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    open_buckets, out = {}, []
    for i, shape in enumerate(shapes):
        shape = tuple(shape)
        bucket = open_buckets.get(shape)
        if bucket is None:
            if len(open_buckets) >= MAX_OPEN_BUCKETS:
                oldest = min(open_buckets, key=lambda k: open_buckets[k][0])
                out.append(open_buckets.pop(oldest))
            bucket = open_buckets[shape] = []
        bucket.append(i)
        if len(bucket) == batch_size:
            out.append(open_buckets.pop(shape))
    out.extend(sorted(open_buckets.values(), key=lambda b: b[0]))
    return out


def letterboxed_shapes(image_files, max_size=None):
    """load_image's output (H, W) of every file, from the image headers alone (nothing is decoded)."""
    shapes = []
    for path in image_files:
        with Image.open(path) as im:
            w, h = im.size
        shapes.append(letterbox_shape((h, w), max_size if max_size is not None else (h, w), auto=True, scaleup=False))
    return shapes


def batch_keys(image_files, max_size=None, output_size="letterbox", denoise="off"):
    """plan_batches' key of every file: its letterboxed (H, W), followed with
    output_size="original" by its own (H, W) -- a batch then holds images of one size, so its
    restored outputs are one [B,H,W,3] tensor -- or else, with denoise="nlm", by its content
    rectangle, which the batch's one denoise launch takes."""
    keys = letterboxed_shapes(image_files, max_size)
    if output_size != "original" and denoise != "nlm":
        return keys
    out = []
    for path, key in zip(image_files, keys):
        with Image.open(path) as im:
            w, h = im.size
        if output_size == "original":
            out.append(tuple(key) + (h, w))
        else:
            out.append(tuple(key) + letterbox_content((h, w), max_size if max_size is not None else (h, w), auto=True,
                                                      scaleup=False))
    return out


class _StageClock:
    """Wall-time sums per pipeline stage, over all threads, into a caller's dict (None: off)."""

    def __init__(self, timings):
        self.timings, self.lock = timings, threading.Lock()

    def add(self, key, t0):
        if self.timings is not None:
            dt = time.perf_counter() - t0
            with self.lock:
                self.timings[key] = self.timings.get(key, 0.0) + dt


_copy_local = threading.local()


def _copy_stream(dev):
    """A side stream per copier thread: its device-to-host copies do not queue behind the next
    batch's launches on the main thread's stream."""
    streams = getattr(_copy_local, "streams", None)
    if streams is None:
        streams = _copy_local.streams = {}
    if dev not in streams:
        streams[dev] = torch.cuda.Stream(dev)
    return streams[dev]


def _write_file(data, save_path, msg):
    with open(save_path, "wb") as fh:
        fh.write(data)
    print(f"{msg}: {save_path}")


class _ImageLines:
    """enhance mode's closing lines of one image, printed once its last file is written."""

    def __init__(self, n_files):
        self.left, self.lock = n_files, threading.Lock()

    def written(self, n):
        with self.lock:
            self.left -= n
            last = self.left == 0
        if last:
            print("图像增强完成！")
            print("-" * 50)


def _write_image_files(files, clock, lines, write_pixels=_write_png):
    t0 = time.perf_counter()
    for data, save_path, msg, encoded in files:
        (_write_file if encoded else write_pixels)(data, save_path, msg)
    if lines is not None:
        lines.written(len(files))
    clock.add("copy_write", t0)


def _finish_batch(job, writer, clock, image_lines, write_pixels=_write_png, trim=False):
    """Copier thread: wait for the batch's event, bring its files (device encoder) or pixels
    (host encoder) to pinned host memory in one copy per tensor, hand the per-image writes to
    the writer threads.  Returns their futures.  write_pixels: the host encoder, or one per
    kind of file.  trim (the device JPEG encoder, whose buffer is
    sized by a bound several times the files): the sizes come first, then only the columns up
    to the longest file."""
    done, dev, outputs, paths = job
    t0 = time.perf_counter()
    done.synchronize()
    clock.add("event_wait", t0)
    t0 = time.perf_counter()
    stream = _copy_stream(dev)
    host = []
    with torch.cuda.stream(stream):
        for msg, u8, buf, sizes in outputs:
            src = buf if buf is not None else u8
            hs = None
            if sizes is not None and trim:
                hs = torch.empty(sizes.shape, dtype=torch.int64, pin_memory=True)
                hs.copy_(sizes, non_blocking=True)
                stream.synchronize()
                src = src[:, :int(hs.max())]
            h = torch.empty(src.shape, dtype=torch.uint8, pin_memory=True)
            h.copy_(src, non_blocking=True)
            if sizes is not None and not trim:
                hs = torch.empty(sizes.shape, dtype=torch.int64, pin_memory=True)
                hs.copy_(sizes, non_blocking=True)
            host.append((msg, h, hs))
    stream.synchronize()
    del outputs, job  # (the device tensors are released after the copies, never before)
    clock.add("copy_write", t0)
    futs = []
    for b, per_kind in enumerate(paths):
        files = []
        for (msg, h, hs), save_path in zip(host, per_kind):
            a = h.numpy()
            if hs is not None:
                files.append((memoryview(a[b, :int(hs[b])]), save_path, msg, True))
            else:
                files.append((a[b], save_path, msg, False))
        lines = _ImageLines(len(files)) if image_lines else None
        if host[0][2] is not None:  # encoded already: one task writes the image's files
            futs.append(writer.submit(_write_image_files, files, clock, lines))
        else:  # PIL encodes: one task per file
            per_file = write_pixels if isinstance(write_pixels, (list, tuple)) else [write_pixels] * len(files)
            futs += [writer.submit(_write_image_files, [f], clock, lines, w) for f, w in zip(files, per_file)]
    return futs


def run_batched(model, image_files, output_dir, device, *, max_size=None, precision="fp32", png_encoder="host",
                batch_size=8, decode_threads=4, clahe=True, comparison=2, image_lines=True, timings=None,
                image_format="png", jpeg_quality=95, output_size="letterbox", guided_radius=4, guided_eps=1e-4,
                jpeg_subsampling="444", jpeg_optimize=False, jpeg_gray_maps=False, denoise="off", denoise_strength=1.0,
                denoise_floor=16, denoise_search=5, denoise_patch=2, denoise_auto_scale=1.0):
    """The batched directory pipeline behind enhance_batch_images(batch_size > 1) and
    main.py --mode predict --infer_batch: for every file {name}_enhanced.png,
    {name}_illumination.png and, unless comparison is None, {name}_comparison.png
    ([input | enhanced] for comparison=2, [input | enhanced | illumination] for 3); .jpg files of
    quality jpeg_quality with image_format="jpg" (host encoder: PIL, device encoders: upr.jpeg;
    jpeg_subsampling and jpeg_optimize for every kind of file, jpeg_gray_maps for the maps).
    clahe: apply_clahe_enhancement after the forward (the enhance mode's default path);
    image_lines: print enhance mode's per-image lines (predict mode prints the saves only).

    plan_batches groups the files by letterboxed shape.  decode_threads PIL threads decode up
    to two batches ahead.  Per batch the main thread queues, on its current stream: one
    staging copy + upr_letterbox_batch in the model's dtype, the forward, CLAHE,
    upr_panels_u8, with a device encoder three batched PNG encodes, and an event.  A copier
    thread waits for the event, copies the files (or, host encoder, the pixels) to pinned
    memory on a side stream and hands the writes (host encoder: PIL encodes) to the writer
    threads.  Two batches are in flight: batch n is queued before batch n - 1 is written and
    after batch n - 2 is.  Every batch has its own staging and output tensors (the allocators
    keep a buffer until the work queued on it has drained); only the PNG scratch is reused,
    stream-ordered.  timings: an optional dict that receives wall-time sums per stage
    (decode_wait, launch, drain_wait on the main thread; event_wait, copy_write over the
    copier and writer threads).

    output_size="original": the files have the source's size.  Batches are keyed by
    (letterboxed shape, original shape) (batch_keys), so mixed sizes form more batches; behind
    upr_panels_u8 a batch runs upr.guided.restore on the staged sources (upr_guided_fit +
    upr_guided_apply, or the crop when nothing was resized) and the encoders take its uniform
    [B,H,W,3] outputs.  A batch's device and pinned host memory then grow with the
    full-resolution pixel count: 3 + 3 * (2 + comparison) bytes per source pixel on the device
    (the staged source and the three outputs) plus the encoders' buffers, not with the
    letterboxed one.

    denoise="nlm": behind upr_panels_u8 one upr.denoise.nlm launch per batch filters the enhanced
    pixels inside the content rectangle (batches are then keyed by that rectangle as well); the
    comparison's enhanced panel is replaced by torch.cat, and with output_size="original" the
    denoised pixels are the restore's target.  denoise_strength="auto": three launches per batch
    instead, on the batch's stream -- upr.denoise.estimate_sigma on the input's u8 pixels (the
    comparison's left panel; without a comparison one more upr_panels_u8 makes them), the
    per-image tables, the filter reading them; the estimates never come to the host."""
    from upr import guided, runtime
    _check_encoder(png_encoder)
    _check_format(image_format, jpeg_quality, jpeg_subsampling, jpeg_optimize, jpeg_gray_maps)
    _check_output_size(output_size, guided_radius, guided_eps)
    dn = _check_denoise(denoise, denoise_strength, denoise_floor, denoise_search, denoise_patch, denoise_auto_scale)
    original = output_size == "original"
    if comparison not in (None, 2, 3):
        raise ValueError(f"comparison must be None, 2 or 3, got {comparison!r}")
    batches = plan_batches(batch_keys(image_files, max_size, output_size, dn.mode), batch_size)
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    dtype = torch.float16 if precision == "fp16" else torch.float32
    adjuster = AdaptiveParameterAdjuster()
    clock = _StageClock(timings)
    decode_threads = max(1, min(int(decode_threads), _BATCH_CPUS - 1))
    writers = max(1, min(_WRITERS, _BATCH_CPUS - decode_threads))
    os.makedirs(output_dir, exist_ok=True)
    kinds = [("enhanced", "已保存"), ("illumination", "已保存")] + ([("comparison", "已保存对比图像")] if comparison else [])
    colour = _Jpeg(jpeg_quality, jpeg_subsampling, jpeg_optimize)
    jpegs = [colour._replace(gray=bool(jpeg_gray_maps)) if kind == "illumination" else colour for kind, _ in kinds]
    n_files, count = len(image_files), 0

    def launch(idxs, images):
        new_shape = max_size if max_size is not None else images[0].shape[:2]
        x = letterbox_u8_batch(images, new_shape, auto=True, scaleup=False, device=dev, dtype=dtype,
                               return_sources=original)
        if original:
            x, sources = x
        with torch.no_grad():
            enh, _, illu = model(x)
        if clahe:
            enh = adjuster.apply_clahe_enhancement(enh)
        content = letterbox_content(images[0].shape[:2], new_shape, auto=True, scaleup=False)
        if original:
            enh_u8, illu_u8, _ = runtime.panels_u8(x, enh, illu, None)
            low_u8 = runtime.panels_u8(x, x, None, None)[0]
            if dn.on:
                enh_u8 = dn.apply(enh_u8, illu_u8, content, low_u8)
            u8s = guided.restore(sources, low_u8, enh_u8, illu_u8, content, guided_radius, guided_eps, comparison)
        else:
            u8s = runtime.panels_u8(x, enh, illu, comparison)
            if dn.on:
                cmp, Wl, low_u8 = u8s[2], x.shape[3], None
                if dn.auto:  # the input's pixels: the comparison's left panel, or a launch of their own
                    low_u8 = cmp[:, :, :Wl] if cmp is not None else runtime.panels_u8(x, x, None, None)[0]
                den = dn.apply(u8s[0], u8s[1], content, low_u8)
                if cmp is not None:  # [input | enhanced (| illumination)]: the middle panel is the denoised one
                    cmp = torch.cat([cmp[:, :, :Wl], den, cmp[:, :, 2 * Wl:]], dim=2)
                u8s = (den, u8s[1], cmp)
        outputs = []
        for (_, msg), u8, jpeg in zip(kinds, u8s, jpegs):
            if png_encoder in _DEVICE_MATCHES:
                buf, sizes = _encode_device(u8, png_encoder, image_format, jpeg)
                outputs.append((msg, None, buf, sizes))
            else:
                outputs.append((msg, u8, None, None))
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(dev))
        names = [os.path.splitext(os.path.basename(image_files[i]))[0] for i in idxs]
        paths = [[os.path.join(output_dir, f"{n}_{kind}.{image_format}") for kind, _ in kinds] for n in names]
        return done, dev, outputs, paths

    def drain(fut):
        t0 = time.perf_counter()
        for w in fut.result():
            w.result()
        clock.add("drain_wait", t0)

    pool = ThreadPoolExecutor(max_workers=decode_threads)
    copier = ThreadPoolExecutor(max_workers=_COPIERS)
    writer = ThreadPoolExecutor(max_workers=writers)
    try:
        todo, decoding, inflight = iter(batches), deque(), deque()

        def decode_ahead():  # the threads work up to two batches ahead of the launches
            while len(decoding) < 2:
                idxs = next(todo, None)
                if idxs is None:
                    return
                decoding.append((idxs, [pool.submit(_decode, image_files[i]) for i in idxs]))

        decode_ahead()
        while decoding:
            idxs, futs = decoding.popleft()
            decode_ahead()
            t0 = time.perf_counter()
            images = [f.result()[0] for f in futs]
            clock.add("decode_wait", t0)
            while len(inflight) >= 2:
                drain(inflight.popleft())
            t0 = time.perf_counter()
            job = launch(idxs, images)
            dt = time.perf_counter() - t0
            clock.add("launch", t0)
            for i in idxs if image_lines else ():
                count += 1
                print(f"[{count}/{n_files}]")
                print(f"正在处理: {os.path.basename(image_files[i])}")
                print(f"增强耗时: {dt / len(idxs):.4f}s")  # the image's share of queueing its batch (no synchronise)
            inflight.append(copier.submit(_finish_batch, job, writer, clock, image_lines,
                                          [_pixel_writer(image_format, j) for j in jpegs], image_format == "jpg"))
            del job
        while inflight:
            drain(inflight.popleft())
    finally:
        pool.shutdown(wait=True, cancel_futures=True)
        copier.shutdown(wait=True)
        writer.shutdown(wait=True)


def enhance_batch_images(input_dir, output_dir, device, max_size=None, use_preact=True, use_aspp=True, seed=None,
                         precision="fp32", png_encoder="host", batch_size=1, decode_threads=4, timings=None,
                         image_format="png", jpeg_quality=95, output_size="letterbox", guided_radius=4,
                         guided_eps=1e-4, jpeg_subsampling="444", jpeg_optimize=False, jpeg_gray_maps=False,
                         denoise="off", denoise_strength=1.0, denoise_floor=16, denoise_search=5, denoise_patch=2,
                         denoise_auto_scale=1.0):
    """Enhance every image of a directory (reference :202-250).

    batch_size=1 (the default) is the reference's one-image-at-a-time loop with a decode
    prefetch and threaded PNG writes.  batch_size > 1 runs the batched path (run_batched;
    decode_threads PIL threads): the same three files per image under the same names and the
    same log lines per image, but the lines come in the order the batches and the writer
    threads produce them, not in listing order (files are grouped by letterboxed shape).  An
    image's files are exactly what the model, apply_clahe_enhancement and to_u8_hwc give for
    the batch tensor the image was placed in (measured on the GPU, no output byte depended on
    that batch: DESIGN.md 4.5).  timings: see run_batched (batched path only).  image_format="jpg"
    writes the three files as .jpg of quality jpeg_quality (jpeg_subsampling, jpeg_optimize and
    jpeg_gray_maps as in enhance_single_image).  output_size="original" writes them
    at each source's size (run_batched / save_original_size; guided_radius, guided_eps).
    denoise="nlm" writes the enhanced pixels denoised (denoise_strength, denoise_floor,
    denoise_search, denoise_patch, denoise_auto_scale as in enhance_single_image; with
    denoise_strength="auto" every image of a batch is filtered at its own measured noise level)."""
    _check_encoder(png_encoder)
    _check_format(image_format, jpeg_quality, jpeg_subsampling, jpeg_optimize, jpeg_gray_maps)
    _check_output_size(output_size, guided_radius, guided_eps)
    dn = _check_denoise(denoise, denoise_strength, denoise_floor, denoise_search, denoise_patch, denoise_auto_scale)
    restore = dict(output_size=output_size, guided_radius=guided_radius, guided_eps=guided_eps,
                   jpeg_subsampling=jpeg_subsampling, jpeg_optimize=jpeg_optimize, jpeg_gray_maps=jpeg_gray_maps,
                   denoise=dn.mode, denoise_strength=dn.public_strength, denoise_floor=dn.floor,
                   denoise_search=dn.search, denoise_patch=dn.patch, denoise_auto_scale=dn.auto_scale)
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    print("正在加载模型...")
    if seed is not None:
        torch.manual_seed(seed)
    model = UP_Retinex(use_preact=use_preact, use_aspp=use_aspp).to(device).eval()
    image_files = list_images(input_dir)
    if not image_files:
        print(f"在目录 '{input_dir}' 中未找到有效图像文件")
        return
    print(f"找到 {len(image_files)} 个图像文件")
    print("=" * 50)
    total = 0.0
    if batch_size > 1:
        t0 = time.time()
        run_batched(model, image_files, output_dir, device, max_size=max_size, precision=precision,
                    png_encoder=png_encoder, batch_size=batch_size, decode_threads=decode_threads, clahe=True,
                    comparison=2, timings=timings, image_format=image_format, jpeg_quality=jpeg_quality, **restore)
        total = time.time() - t0
        return _print_totals(len(image_files), total)
    # host pipeline around the device work: the next file is decoded on a
    # prefetch thread and the PNG encodes run on writer threads while the GPU
    # enhances the current image (the reference does all three serially)
    with ThreadPoolExecutor(max_workers=1) as reader, ThreadPoolExecutor(max_workers=_WRITERS) as writer:
        nxt = reader.submit(_decode, image_files[0])
        for i, path in enumerate(image_files, 1):
            print(f"[{i}/{len(image_files)}]")
            t0 = time.time()
            decoded = nxt.result()
            if i < len(image_files):
                nxt = reader.submit(_decode, image_files[i])
            enhance_single_image(model, path, output_dir, device, max_size, precision=precision, _decoded=decoded,
                                 _writer=writer, png_encoder=png_encoder, image_format=image_format,
                                 jpeg_quality=jpeg_quality, **restore)
            total += time.time() - t0
            print("-" * 50)
    _print_totals(len(image_files), total)


def _print_totals(n, total):
    print("=" * 50)
    print(f"总共处理了 {n} 张图像")
    print(f"总耗时: {total:.2f}s")
    print(f"平均每张图像耗时: {total / n:.4f}s")
    print("=" * 50)
