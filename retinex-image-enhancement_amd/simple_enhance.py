#!/usr/bin/env python3
"""Root enhance CLI (drop-in for the reference simple_enhance.py:17-94):
--input/--output/--max_size/--device/--multi_scale/--content_aware, plus --seed and
--output_size {letterbox,original} with --guided_radius / --guided_eps (original: the files
have the source's size, upr.guided), and --image_format {png,jpg} with --jpeg_quality,
--jpeg_subsampling {444,420}, --jpeg_optimize and --jpeg_gray_maps (jpg: the three files as
JPEGs, as main.py's flags of the same names), and --denoise {off,nlm} with --denoise_strength /
--denoise_floor / --denoise_search / --denoise_patch (nlm: the enhanced pixels are denoised
before they are written, upr.denoise; --denoise_strength auto measures each image's noise
level on the device and filters with --denoise_auto_scale times it)."""
import argparse
import os
import sys
from pathlib import Path

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from enhancers.simple_enhance import enhance_single_image, enhance_batch_images  # noqa: E402
from models.model import UP_Retinex  # noqa: E402


def _strength(text):
    if text == 'auto':
        return text
    try:
        return float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"must be a number or 'auto', got {text!r}")


def build_parser():
    ap = argparse.ArgumentParser(description='简化版UP-Retinex图像增强工具 (MI355X)')
    ap.add_argument('--input', type=str, required=True)
    ap.add_argument('--output', type=str, default='./results')
    ap.add_argument('--max_size', type=int, default=None)
    ap.add_argument('--device', type=str, default=None)
    ap.add_argument('--multi_scale', action='store_true')
    ap.add_argument('--content_aware', action='store_true')
    ap.add_argument('--seed', type=int, default=None)
    ap.add_argument('--output_size', choices=['letterbox', 'original'], default='letterbox',
                    help='size of the output files: the letterboxed tensor\'s (default) or the source\'s '
                         '(guided-filter restore)')
    ap.add_argument('--guided_radius', type=int, default=4, help='--output_size original: window radius, 1..32')
    ap.add_argument('--guided_eps', type=float, default=1e-4, help='--output_size original: regulariser, > 0')
    ap.add_argument('--image_format', choices=['png', 'jpg'], default='png', help='format of the output files')
    ap.add_argument('--jpeg_quality', type=int, default=95, help='--image_format jpg: quality 1..100')
    ap.add_argument('--jpeg_subsampling', choices=['444', '420'], default='444',
                    help='--image_format jpg: chroma subsampling of the three files')
    ap.add_argument('--jpeg_optimize', action='store_true', help='--image_format jpg: Huffman tables built per file')
    ap.add_argument('--jpeg_gray_maps', action='store_true',
                    help='--image_format jpg: write _illumination.jpg as a one-component (grayscale) file')
    ap.add_argument('--denoise', choices=['off', 'nlm'], default='off',
                    help='nlm: denoise the enhanced image\'s u8 pixels before they are written (non-local means, '
                         'stronger where the illumination map is darker)')
    ap.add_argument('--denoise_strength', type=_strength, default=1.0,
                    help='--denoise nlm: assumed noise std of the input in u8 levels, >= 0, or `auto`: measured per '
                         'image on the device')
    ap.add_argument('--denoise_auto_scale', type=float, default=1.0,
                    help='--denoise_strength auto: multiplies the estimate, >= 0')
    ap.add_argument('--denoise_floor', type=int, default=16,
                    help='--denoise nlm: the illumination level below which the strength stops growing, 1..255')
    ap.add_argument('--denoise_search', type=int, default=5, help='--denoise nlm: search radius, 1..10')
    ap.add_argument('--denoise_patch', type=int, default=2, help='--denoise nlm: patch radius, 1..3')
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    restore = dict(output_size=args.output_size, guided_radius=args.guided_radius, guided_eps=args.guided_eps,
                   denoise=args.denoise, denoise_strength=args.denoise_strength, denoise_floor=args.denoise_floor,
                   denoise_search=args.denoise_search, denoise_patch=args.denoise_patch,
                   denoise_auto_scale=args.denoise_auto_scale,
                   image_format=args.image_format, jpeg_quality=args.jpeg_quality,
                   jpeg_subsampling=args.jpeg_subsampling, jpeg_optimize=args.jpeg_optimize,
                   jpeg_gray_maps=args.jpeg_gray_maps)
    if args.device is None:
        args.device = 'cuda' if torch.cuda.is_available() else 'cpu'
    print(f"使用设备: {args.device}")
    if not os.path.exists(args.input):
        print(f"错误: 找不到输入路径 '{args.input}'")
        return
    p = Path(args.input)
    if p.is_file():
        if args.seed is not None:
            torch.manual_seed(args.seed)
        model = UP_Retinex().to(args.device).eval()
        # the reference passes only enable_multi_scale here (--content_aware is ignored, :66-77)
        enhance_single_image(model=model, image_path=str(p), output_dir=args.output, device=args.device,
                             max_size=args.max_size, enable_multi_scale=args.multi_scale, **restore)
    elif p.is_dir():
        enhance_batch_images(input_dir=str(p), output_dir=args.output, device=args.device, max_size=args.max_size,
                             seed=args.seed, **restore)
    else:
        print(f"错误: 输入路径 '{args.input}' 不是有效的文件或目录")
        return
    print(f"结果已保存到: {args.output}")


if __name__ == "__main__":
    main()
