#!/usr/bin/env python3
"""UP-Retinex CLI (drop-in for the reference main.py; same flags, same modes).

`--mode enhance` is the hot path: every image runs the fused gfx950 graph
(libupr.so) and the device-side enhancers.  Additions: --seed (the reference
never seeds its random init, main.py:229), --precision {fp32,fp16} and
--png_encoder {host,device,device_lz} (enhance / predict: PIL on the host, the
default, or the device-side encoder of upr.png -- same pixels, no host encode;
device is Huffman-only and writes larger files, device_lz adds LZ77 matching).
--image_format {png,jpg} and --jpeg_quality Q (additions, default png / 95):
jpg writes the enhance / predict outputs as baseline 4:4:4 JPEGs, PIL's with
--png_encoder host, the device encoder's (upr.jpeg) with device or device_lz.
--jpeg_subsampling {444,420} (default 444), --jpeg_optimize and --jpeg_gray_maps
(additions, jpg only): 4:2:0 chroma and per-file Huffman tables for every file,
the illumination map as a one-component file.
Intentional divergences (reference bugs): a single-file --mode enhance works
(reference main.py:240-249 raises TypeError); --mode predict unpacks the
model's 3-tuple (reference predict.py:163 raises ValueError).
--output_size {letterbox,original} (an addition, default letterbox) with
--guided_radius R / --guided_eps E: original writes the enhance / predict files
at the source's size -- the letterboxed result carried to the decoded pixels by
the guided-filter restore (upr.guided), the bars cropped away.
--denoise {off,nlm} (an addition, default off) with --denoise_strength /
--denoise_floor / --denoise_search / --denoise_patch: nlm writes the enhance /
predict files with the enhanced pixels denoised by the illumination-weighted
non-local means of upr.denoise (the illumination file does not change).
--denoise_strength auto measures each image's noise level on the device and
filters with --denoise_auto_scale times it.
--infer_batch N (an addition, default 1) runs --mode enhance / predict on a
directory N images at a time (enhancers/simple_enhance.py run_batched).
--mode train runs trainers.train.train(args): images of --train_dir are decoded
on host threads, letterboxed and augmented on the device (datasets/dataset.py),
and every step runs on the HIP path (train_step, losses/loss.py TotalLoss,
upr.optim.Adam); schedulers, early stopping, latest_model.pth / best_model.pth
and results.csv follow the reference (trainers/train.py:189-396).  --seed also
seeds the shuffle, the augmentation draws and the noise generator.
--mode evaluate (an addition) runs no model: the image-quality metrics of
utils/utils.py for every image of --input_path, against --reference_dir when
given, written to <output_dir>/metrics.csv.  --lowlight_dir DIR (an addition)
adds a last column `loe`, the lightness order error (Wang et al. 2013) of each
image against its low-light source on a --loe_size grid (default 50).
--val_dir DIR (an addition, --mode train) validates on held-out images after
every --val_freq-th epoch (trainers.train.validate: eval-mode fp32 forward,
TotalLoss forward only, the metrics and LOE; --val_reference_dir adds psnr /
ssim / mse), appends val_* columns to results.csv, lets --best_by choose what
picks best_model.pth, and writes --val_samples comparison panels under
<save_dir>/samples/.
--train_reference_dir DIR (an addition, --mode train) trains on pairs: the ground
truth of every --train_dir file is the file of DIR with its stem, and the
Charbonnier and 1 - SSIM terms against it join the loss under --weight_rec /
--weight_ssim (default 1.0 each; --rec_eps 1e-3) and results.csv as the columns
reconstruction and ssim_loss.
"""
import argparse
import os
import sys
from pathlib import Path

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from models.model import UP_Retinex  # noqa: E402
from enhancers.simple_enhance import (enhance_single_image, enhance_batch_images, list_images,  # noqa: E402
                                      load_image, save_image, create_comparison, run_batched, save_original_size,
                                      save_denoised, _decode)
from enhancers.adaptive_params import AdaptiveParameterAdjuster  # noqa: E402
from utils.letterbox import letterbox_content  # noqa: E402


def _jpeg_quality(text):
    q = int(text)
    if not 1 <= q <= 100:
        raise argparse.ArgumentTypeError(f"must be in 1..100, got {text}")
    return q


def _int_at_least(lo):
    def parse(text):
        v = int(text)
        if v < lo:
            raise argparse.ArgumentTypeError(f"must be >= {lo}, got {text}")
        return v
    return parse


_positive, _non_negative = _int_at_least(1), _int_at_least(0)


def _strength(text):
    """--denoise_strength: a number, or `auto`."""
    if text == 'auto':
        return text
    try:
        return float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"must be a number or 'auto', got {text!r}")


def build_parser():
    p = argparse.ArgumentParser(description='UP-Retinex: 基于Retinex理论的低光照图像增强 (MI355X)')
    p.add_argument('--mode', type=str, choices=['train', 'predict', 'enhance', 'evaluate'], default='predict')
    p.add_argument('--train_dir', type=str, default='./data/train')
    p.add_argument('--test_dir', type=str, default='./data/test')
    p.add_argument('--input_path', type=str, default='./data/test')
    p.add_argument('--output_dir', type=str, default='./results')
    p.add_argument('--checkpoint', type=str, default='./checkpoints/best_model.pth')
    p.add_argument('--save_dir', type=str, default='./checkpoints')
    p.add_argument('--num_epochs', type=int, default=100)
    p.add_argument('--batch_size', type=int, default=8)
    p.add_argument('--image_size', type=int, default=640)
    p.add_argument('--lr', type=float, default=1e-4)
    p.add_argument('--weight_decay', type=float, default=1e-5)
    p.add_argument('--resume', type=str, default=None)
    p.add_argument('--weight_exp', type=float, default=10.0)
    p.add_argument('--weight_smooth', type=float, default=1.0)
    p.add_argument('--weight_col', type=float, default=0.5)
    p.add_argument('--weight_spa', type=float, default=1.0)
    p.add_argument('--weight_decouple', type=float, default=0.1)
    p.add_argument('--weight_perceptual', type=float, default=1.0)
    p.add_argument('--weight_freq', type=float, default=0.5)
    p.add_argument('--max_size', type=int, default=None)
    p.add_argument('--no_comparison', action='store_true')
    p.add_argument('--device', type=str, default=None)
    p.add_argument('--multi_scale', action='store_true')
    p.add_argument('--content_aware', action='store_true')
    p.add_argument('--num_workers', type=int, default=4)
    p.add_argument('--lr_decay_step', type=int, default=30)
    p.add_argument('--lr_decay_gamma', type=float, default=0.5)
    p.add_argument('--save_freq', type=int, default=10)
    p.add_argument('--use_amp', action='store_true')
    p.add_argument('--patience', type=int, default=20)
    p.add_argument('--use_cosine_scheduler', action='store_true')
    p.add_argument('--use_freq_loss', action='store_true')
    p.add_argument('--adaptive_weights', action='store_true')
    p.add_argument('--use_preact', action='store_true')
    p.add_argument('--use_aspp', action='store_true')
    p.add_argument('--advanced_augment', action='store_true')
    # additions
    p.add_argument('--seed', type=int, default=None, help='seed the random init (reproducible outputs)')
    p.add_argument('--precision', choices=['fp32', 'fp16'], default='fp32')
    p.add_argument('--png_encoder', choices=['host', 'device', 'device_lz'], default='host',
                   help='--mode enhance / predict: who encodes the PNGs (device: lossless, larger files; '
                        'device_lz: the device encoder with LZ77 matching)')
    p.add_argument('--image_format', choices=['png', 'jpg'], default='png',
                   help='--mode enhance / predict: format of the output files (jpg: baseline 4:4:4 JPEG; '
                        '--png_encoder chooses PIL or the device encoder for it as well)')
    p.add_argument('--jpeg_quality', type=_jpeg_quality, default=95,
                   help='--image_format jpg: quality 1..100, as PIL\'s `quality`')
    p.add_argument('--jpeg_subsampling', choices=['444', '420'], default='444',
                   help='--image_format jpg: chroma subsampling of the three files (420: PIL\'s default)')
    p.add_argument('--jpeg_optimize', action='store_true',
                   help='--image_format jpg: Huffman tables built per file (PIL\'s optimize=True)')
    p.add_argument('--jpeg_gray_maps', action='store_true',
                   help='--image_format jpg: write _illumination.jpg as a one-component (grayscale) file')
    p.add_argument('--output_size', choices=['letterbox', 'original'], default='letterbox',
                   help='--mode enhance / predict: size of the output files: the letterboxed tensor\'s (default) '
                        'or the source\'s (guided-filter restore of the result to the decoded image)')
    p.add_argument('--guided_radius', type=int, default=4, help='--output_size original: window radius, 1..32')
    p.add_argument('--guided_eps', type=float, default=1e-4, help='--output_size original: regulariser, > 0')
    p.add_argument('--denoise', choices=['off', 'nlm'], default='off',
                   help='--mode enhance / predict: nlm denoises the enhanced image\'s u8 pixels before they are '
                        'written (non-local means, stronger where the illumination map is darker)')
    p.add_argument('--denoise_strength', type=_strength, default=1.0,
                   help='--denoise nlm: assumed noise std of the input in u8 levels, >= 0, or `auto`: measured per '
                        'image on the device (upr.denoise.estimate_sigma)')
    p.add_argument('--denoise_auto_scale', type=float, default=1.0,
                   help='--denoise_strength auto: multiplies the estimate, >= 0 (a Laplacian estimator reads low on '
                        'noise that demosaicing or JPEG has correlated)')
    p.add_argument('--denoise_floor', type=int, default=16,
                   help='--denoise nlm: the illumination level below which the strength stops growing, 1..255')
    p.add_argument('--denoise_search', type=int, default=5, help='--denoise nlm: search radius, 1..10')
    p.add_argument('--denoise_patch', type=int, default=2, help='--denoise nlm: patch radius, 1..3')
    p.add_argument('--infer_batch', type=int, default=1,
                   help='--mode enhance / predict on a directory: images per batch (1: one image at a time; '
                        '> 1: the batched path, files grouped by letterboxed shape, --num_workers decode threads; '
                        'a single-file input ignores it)')
    p.add_argument('--reference_dir', type=str, default=None,
                   help='--mode evaluate: ground-truth images, matched by file stem (adds psnr / ssim / mse)')
    p.add_argument('--lowlight_dir', type=str, default=None,
                   help='--mode evaluate: the low-light sources, matched by file stem (adds the lightness order '
                        'error column `loe`)')
    p.add_argument('--noise_sigma', action='store_true',
                   help='--mode evaluate: adds a last column `noise_sigma`, the blind noise estimate of each image in '
                        'u8 levels (utils.utils.batch_noise_sigma)')
    p.add_argument('--loe_size', type=_non_negative, default=50,
                   help='--lowlight_dir / --val_dir: LOE sample grid, pixels on the shorter side (0: every pixel)')
    p.add_argument('--val_dir', type=str, default=None,
                   help='--mode train: held-out low-light images; validation after every --val_freq-th epoch')
    p.add_argument('--val_reference_dir', type=str, default=None,
                   help='--val_dir: ground truth matched by file stem (adds val_psnr / val_ssim / val_mse)')
    p.add_argument('--val_freq', type=_positive, default=1,
                   help='--val_dir: validate after every N-th epoch and always after the last epoch run')
    p.add_argument('--val_batch_size', type=_positive, default=None, help='--val_dir: default --batch_size')
    p.add_argument('--best_by', choices=['train_total', 'val_total', 'val_psnr', 'val_loe'], default='train_total',
                   help='--mode train: the number that picks best_model.pth and drives --patience (val_psnr: '
                        'higher is better; val_* need --val_dir, val_psnr --val_reference_dir)')
    p.add_argument('--val_samples', type=_non_negative, default=4,
                   help='--val_dir: [input | enhanced | illumination] panels of the first K validation images under '
                        '<save_dir>/samples/epoch_NNNN/ on validated --save_freq epochs and the last (0: none)')
    p.add_argument('--train_reference_dir', type=str, default=None,
                   help='--mode train: ground truth of --train_dir matched by file stem; training adds the paired '
                        'terms reconstruction (Charbonnier) and ssim_loss (1 - SSIM) against it')
    p.add_argument('--weight_rec', type=float, default=None,
                   help='--train_reference_dir: weight of the reconstruction term (default 1.0)')
    p.add_argument('--weight_ssim', type=float, default=None,
                   help='--train_reference_dir: weight of the ssim_loss term (default 1.0)')
    p.add_argument('--rec_eps', type=float, default=1e-3, help='--train_reference_dir: the Charbonnier eps')
    return p


def parse_args(argv=None):
    """build_parser().parse_args plus the checks that span flags (an argument
    error, before anything touches the device)."""
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.best_by.startswith('val_') and not args.val_dir:
        parser.error(f"--best_by {args.best_by} needs --val_dir")
    if args.best_by == 'val_psnr' and not args.val_reference_dir:
        parser.error("--best_by val_psnr needs --val_reference_dir")
    if args.train_reference_dir is None:
        for flag, v in (('--weight_rec', args.weight_rec), ('--weight_ssim', args.weight_ssim)):
            if v is not None:
                parser.error(f"{flag} needs --train_reference_dir")
    else:
        args.weight_rec = 1.0 if args.weight_rec is None else args.weight_rec
        args.weight_ssim = 1.0 if args.weight_ssim is None else args.weight_ssim
    if args.val_reference_dir and not args.val_dir:
        parser.error("--val_reference_dir needs --val_dir")
    try:
        from upr import denoise
        denoise.check_params(args.denoise_strength, args.denoise_floor, args.denoise_search, args.denoise_patch,
                             args.denoise_auto_scale)
    except ValueError as e:
        parser.error(str(e))
    return args


def _model(args):
    if args.seed is not None:
        torch.manual_seed(args.seed)
    m = UP_Retinex(use_preact=args.use_preact, use_aspp=args.use_aspp)
    return m


def _place(model, args):
    # compute precision follows the input tensor's dtype (fp16 inputs run the fp16 graph)
    return model.to(args.device).eval()


def _output_format(args):
    return dict(png_encoder=args.png_encoder, image_format=args.image_format, jpeg_quality=args.jpeg_quality,
                jpeg_subsampling=args.jpeg_subsampling, jpeg_optimize=args.jpeg_optimize,
                jpeg_gray_maps=args.jpeg_gray_maps)


def _denoise(args):
    return dict(denoise=args.denoise, denoise_strength=args.denoise_strength, denoise_floor=args.denoise_floor,
                denoise_search=args.denoise_search, denoise_patch=args.denoise_patch,
                denoise_auto_scale=args.denoise_auto_scale)


def _restore(args):
    return dict(output_size=args.output_size, guided_radius=args.guided_radius, guided_eps=args.guided_eps,
                **_denoise(args))


def _predict_one(model, path, args):
    """predictors/predict.py:144-191 predict_single_image: enhanced, illumination
    and the 3-panel [input | enhanced | illumination] comparison (:102-140; the
    1-channel map's channel mean is the map itself, replicated to RGB)."""
    decoded = _decode(path)
    x, _ = load_image(path, args.max_size, decoded=decoded)
    x = x.to(args.device)
    if args.precision == 'fp16':
        x = x.half()
    with torch.no_grad():
        enh, _, illu = model(x)
    os.makedirs(args.output_dir, exist_ok=True)
    name = os.path.splitext(os.path.basename(path))[0]
    enc, ext = _output_format(args), args.image_format
    if args.output_size == 'original':
        save_original_size(decoded[0], x, enh, illu,
                           [os.path.join(args.output_dir, f"{name}_{kind}.{ext}")
                            for kind in ("enhanced", "illumination", "comparison")], args.max_size,
                           None if args.no_comparison else 3, guided_radius=args.guided_radius,
                           guided_eps=args.guided_eps, **enc, **_denoise(args))
        return
    if args.denoise == 'nlm':
        shape = decoded[0].shape[:2]
        save_denoised(x, enh, illu,
                      [os.path.join(args.output_dir, f"{name}_{kind}.{ext}")
                       for kind in ("enhanced", "illumination", "comparison")],
                      letterbox_content(shape, args.max_size if args.max_size is not None else shape, auto=True,
                                        scaleup=False),
                      None if args.no_comparison else 3, **enc, **_denoise(args))
        return
    save_image(enh, os.path.join(args.output_dir, f"{name}_enhanced.{ext}"), **dict(enc, jpeg_gray_maps=False))
    save_image(illu, os.path.join(args.output_dir, f"{name}_illumination.{ext}"), **enc)
    if not args.no_comparison:
        create_comparison(x, enh, os.path.join(args.output_dir, f"{name}_comparison.{ext}"), illu_map=illu, **enc)


def _reference_stems(reference_dir):
    by_stem = {}
    for f in list_images(reference_dir):
        by_stem.setdefault(Path(f).stem, f)
    return by_stem


def _reference_for(path, reference_dir, by_stem=None):
    """The ground truth of NAME.ext: the file of --reference_dir with stem NAME,
    else with NAME's trailing `_enhanced` removed."""
    stem = Path(path).stem
    stems = [stem] + ([stem[:-len('_enhanced')]] if stem.endswith('_enhanced') else [])
    if by_stem is None:
        by_stem = _reference_stems(reference_dir)
    for s in stems:
        if s in by_stem:
            return by_stem[s]
    raise ValueError(f"no reference image for '{path}' in '{reference_dir}' (looked for stem "
                     f"{' or '.join(repr(s) for s in stems)})")


def evaluate(args):
    """Metrics of every image of --input_path (utils.utils.batch_metrics) -> <output_dir>/metrics.csv:
    `file`, then the metric names in calculate_metrics' order; one row per image
    (values as repr(float)) and a last row `mean` of the column means.
    Consecutive images of one size share a launch, up to --batch_size.
    With --lowlight_dir a last column `loe` (utils.utils.batch_loe, --loe_size)
    measures each image against its low-light source, matched by stem like the
    ground truth.  With --noise_sigma a last column `noise_sigma` (after `loe`):
    utils.utils.batch_noise_sigma of each image."""
    from utils.utils import batch_loe, batch_metrics, batch_noise_sigma, metric_names
    p = Path(args.input_path)
    files = [str(p)] if p.is_file() else (list_images(str(p)) if p.is_dir() else None)
    if not files:
        print(f"错误: 输入路径 '{args.input_path}' 不存在")
        return None
    paired = args.reference_dir is not None
    lowlight = getattr(args, 'lowlight_dir', None)
    noise = bool(getattr(args, 'noise_sigma', False))
    names = metric_names(paired) + (('loe',) if lowlight else ()) + (('noise_sigma',) if noise else ())
    by_stem = _reference_stems(args.reference_dir) if paired else None
    low_by_stem = _reference_stems(lowlight) if lowlight else None
    cols = []  # per launch: [n_metrics, b] device tensors

    def flush(xs, ys, ls):
        if xs:
            x = torch.cat(xs)
            m = batch_metrics(x, torch.cat(ys) if paired else None)
            if lowlight:
                m['loe'] = batch_loe(torch.cat(ls), x, args.loe_size)
            if noise:
                m['noise_sigma'] = batch_noise_sigma(x)
            cols.append(torch.stack([m[n] for n in names]))

    xs, ys, ls = [], [], []
    for f in files:
        x, _ = load_image(f, args.max_size, device=args.device)
        y = low = None
        if paired:
            rf = _reference_for(f, args.reference_dir, by_stem)
            y, _ = load_image(rf, args.max_size, device=args.device)
            if y.shape != x.shape:
                raise ValueError(f"reference '{rf}' is {tuple(y.shape[2:])} after loading, '{f}' is "
                                 f"{tuple(x.shape[2:])}")
        if lowlight:
            lf = _reference_for(f, lowlight, low_by_stem)
            low, _ = load_image(lf, args.max_size, device=args.device)
            if low.shape != x.shape:
                raise ValueError(f"low-light image '{lf}' is {tuple(low.shape[2:])} after loading, '{f}' is "
                                 f"{tuple(x.shape[2:])}")
        if xs and (x.shape != xs[0].shape or len(xs) >= max(1, args.batch_size)):
            flush(xs, ys, ls)
            xs, ys, ls = [], [], []
        xs.append(x)
        ys.append(y)
        ls.append(low)
    flush(xs, ys, ls)
    table = torch.cat(cols, dim=1).t().cpu().tolist()  # the one device-to-host copy
    means = [sum(r[k] for r in table) / len(table) for k in range(len(names))]
    os.makedirs(args.output_dir, exist_ok=True)
    out = os.path.join(args.output_dir, 'metrics.csv')
    with open(out, 'w') as fh:
        fh.write(','.join(('file',) + tuple(names)) + '\n')
        for f, r in zip(files, table):
            fh.write(','.join([os.path.basename(f)] + [repr(float(v)) for v in r]) + '\n')
        fh.write(','.join(['mean'] + [repr(float(v)) for v in means]) + '\n')
    print(f"评估完成: {len(files)} 张图像, " + ', '.join(f"{n}={v:.4f}" for n, v in zip(names, means)) + f" -> {out}")
    return out


def main(argv=None):
    args = parse_args(argv)
    if args.device is None:
        args.device = 'cuda' if torch.cuda.is_available() else 'cpu'
    print(f"使用设备: {args.device}")
    print(f"运行模式: {args.mode}")
    if args.mode == 'train':
        from trainers.train import train
        train(args)
        return
    if args.mode == 'evaluate':
        evaluate(args)
        return
    if args.mode == 'predict':
        if not os.path.exists(args.checkpoint):
            print(f"错误: 找不到模型检查点文件 '{args.checkpoint}'")
            return
        model = _model(args)
        ckpt = torch.load(args.checkpoint, map_location='cpu', weights_only=True)
        model.load_state_dict(ckpt['model_state_dict'])
        model = _place(model, args)
        p = Path(args.input_path)
        files = [str(p)] if p.is_file() else (list_images(str(p)) if p.is_dir() else None)
        if files is None:
            print(f"错误: 输入路径 '{args.input_path}' 不存在")
            return
        if p.is_dir() and args.infer_batch > 1:
            run_batched(model, files, args.output_dir, args.device, max_size=args.max_size, precision=args.precision,
                        batch_size=args.infer_batch, decode_threads=args.num_workers, clahe=False,
                        comparison=None if args.no_comparison else 3, image_lines=False, **_output_format(args),
                        **_restore(args))
        else:
            for f in files:
                _predict_one(model, f, args)
        print("推理完成，结果已保存到:", args.output_dir)
        return
    # enhance
    os.makedirs(args.output_dir, exist_ok=True)
    p = Path(args.input_path)
    if p.is_file():
        model = _place(_model(args), args)
        enhance_single_image(model=model, image_path=str(p), output_dir=args.output_dir, device=args.device,
                             max_size=args.max_size, adjuster=AdaptiveParameterAdjuster(),
                             enable_multi_scale=args.multi_scale, enable_content_aware=args.content_aware,
                             precision=args.precision, **_output_format(args), **_restore(args))
    elif p.is_dir():
        # reference: enhance_batch_images builds UP_Retinex() with its defaults (preact + ASPP)
        enhance_batch_images(input_dir=str(p), output_dir=args.output_dir, device=args.device,
                             max_size=args.max_size, seed=args.seed, precision=args.precision,
                             batch_size=args.infer_batch, decode_threads=args.num_workers, **_output_format(args),
                             **_restore(args))
    else:
        print(f"错误: 输入路径 '{args.input_path}' 不存在")
        return
    print("图像增强完成，结果已保存到:", args.output_dir)


if __name__ == '__main__':
    main()
