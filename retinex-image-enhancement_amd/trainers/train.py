"""UP-Retinex training (drop-in for the reference trainers/train.py): the step
(:27-131) and, below it, the epoch driver train(args) with its schedulers,
checkpoint files, early stopping and results.csv (:134-396, :520-600).

`train_one_epoch` keeps the reference's signature and step order
(zero_grad -> forward -> TotalLoss -> backward -> clip_grad_norm_(1.0) ->
Adam.step()); the model, loss and optimiser it is handed run on the gfx950
training kernels: `make_optimizer` builds upr.optim.Adam (flat-buffer fused
clip + Adam), and `clip_grad_norm_` is upr.optim's.  With `use_amp` and a
scaler the step follows the reference's AMP branch (train.py:71-89): scaled
backward, unscale_ (one launch over the flat gradient buffer), clip, a step
skipped on inf/nan, scale update — upr.amp.GradScaler (a torch.amp.GradScaler
handed in is mirrored by one with its settings).  As in the reference, the
forward and the loss of that branch run under torch.autocast: the engine then
computes its MFMA convolutions (and their input gradients) in fp16 with fp32
accumulation (upr/train/, autocast_active); weight gradients, BatchNorm, the
losses and the optimiser stay fp32.  `amp_fp16=False` keeps the GradScaler
control flow with fp32 arithmetic.
"""
import csv
import math
import os
import time
from datetime import datetime

import torch

from losses.loss import deferred_readback
from upr import amp as uamp
from upr import optim as uoptim

clip_grad_norm_ = uoptim.clip_grad_norm_
GradScaler = uamp.GradScaler
_mirrors = {}


def _as_upr_scaler(scaler):
    if scaler is None or isinstance(scaler, uamp.GradScaler):
        return scaler
    m = _mirrors.get(id(scaler))
    if m is None or m[0] is not scaler:
        m = _mirrors[id(scaler)] = (scaler, uamp.GradScaler.from_torch(scaler))
    return m[1]


def make_optimizer(model, lr=1e-4, weight_decay=1e-5):
    """optim.Adam(model.parameters(), lr, weight_decay) of train.py:241-245."""
    return uoptim.Adam(model.parameters(), lr=lr, weight_decay=weight_decay)


def train_step(model, img_low, criterion, optimizer, max_norm=1.0, scaler=None, use_amp=False, grad_hook=None,
               amp_fp16=True, target=None):
    """One step body (train.py:63-103).  Returns (loss, loss_dict).  grad_hook
    (e.g. upr.dist.allreduce_grads for data parallelism) runs between the
    backward and the unscale / clip.  target (an addition): the batch's ground
    truth, handed to the criterion (TotalLoss's paired terms)."""
    optimizer.zero_grad()
    scaler = _as_upr_scaler(scaler) if use_amp else None
    # the loss_dict's floats are read back after the backward / optimizer work is
    # queued (returned materialised), not between forward and backward
    with torch.autocast("cuda", dtype=torch.float16, enabled=scaler is not None and amp_fp16), \
            deferred_readback():
        img_enhanced, reflectance, illu_map = model(img_low)
        if target is None:
            loss, loss_dict = criterion(img_low, img_enhanced, illu_map, reflectance)
        else:
            loss, loss_dict = criterion(img_low, img_enhanced, illu_map, reflectance, target=target)
    if scaler is not None:
        scaler.scale(loss).backward()
        if grad_hook is not None:
            grad_hook()
        scaler.unscale_(optimizer)
        clip_grad_norm_(model.parameters(), max_norm=max_norm)
        scaler.step(optimizer)
        scaler.update()
    else:
        loss.backward()
        if grad_hook is not None:
            grad_hook()
        clip_grad_norm_(model.parameters(), max_norm=max_norm)
        optimizer.step()
    return loss, (dict(loss_dict.items()) if type(loss_dict) is not dict else loss_dict)


def train_one_epoch(model, dataloader, criterion, optimizer, device, epoch, writer=None, scaler=None, use_amp=False):
    """A batch of the loader is a low-light tensor, or a (low, target) pair of a
    paired loader: the averages then carry PAIRED_KEYS too."""
    model.train()
    keys = ('total', 'exposure', 'smoothness', 'color', 'spatial', 'decouple', 'perceptual')
    totals = {k: 0.0 for k in keys}
    n = 0
    t0 = time.time()
    for batch_idx, batch in enumerate(dataloader):
        img_low, target = batch if isinstance(batch, (tuple, list)) else (batch, None)
        img_low = img_low.to(device, torch.float32)
        if target is not None:
            target = target.to(device, torch.float32)
        _, loss_dict = train_step(model, img_low, criterion, optimizer, scaler=scaler, use_amp=use_amp, target=target)
        for k in keys + (PAIRED_KEYS if target is not None else ()):
            totals[k] = totals.get(k, 0.0) + loss_dict[k]
        n += 1
        if writer is not None and batch_idx % 100 == 0:
            for k, v in loss_dict.items():
                writer.add_scalar(f'Loss/{k}', v, epoch * max(1, len(dataloader)) + batch_idx)
    if n:
        totals = {k: v / n for k, v in totals.items()}
    totals["_epoch_seconds"] = time.time() - t0
    return totals


# ---- the epoch driver (reference trainers/train.py:134-396, :520-600) --------
LOSS_KEYS = ('total', 'exposure', 'smoothness', 'color', 'spatial', 'decouple', 'perceptual')
# the columns a paired run (--train_reference_dir) adds after them
PAIRED_KEYS = ('reconstruction', 'ssim_loss')


class StepLR:
    """torch.optim.lr_scheduler.StepLR for upr.optim.Adam (which is no
    torch.optim.Optimizer): step() sets param_groups[0]['lr'] to its closed form
    base_lr * gamma ** (last_epoch // step_size).  base_lr is the lr the
    optimizer was built with; last_epoch > 0 continues a resumed run in phase."""

    def __init__(self, optimizer, step_size, gamma=0.1, last_epoch=0, base_lr=None):
        self.optimizer, self.step_size, self.gamma = optimizer, int(step_size), float(gamma)
        self.base_lr = float(optimizer.param_groups[0]['lr'] if base_lr is None else base_lr)
        self.last_epoch = int(last_epoch)
        self._apply()

    def get_lr(self):
        return self.base_lr * self.gamma ** (self.last_epoch // self.step_size)

    def _apply(self):
        self.optimizer.param_groups[0]['lr'] = self.get_lr()

    def step(self):
        self.last_epoch += 1
        self._apply()


class CosineAnnealingWarmRestarts(StepLR):
    """torch.optim.lr_scheduler.CosineAnnealingWarmRestarts, stepped once per
    epoch: eta_min + (base_lr - eta_min) * (1 + cos(pi * T_cur / T_i)) / 2 with
    (T_cur, T_i) the position in the current restart period, from last_epoch."""

    def __init__(self, optimizer, T_0=10, T_mult=2, eta_min=1e-6, last_epoch=0, base_lr=None):
        self.T_0, self.T_mult, self.eta_min = int(T_0), int(T_mult), float(eta_min)
        super().__init__(optimizer, 1, 1.0, last_epoch, base_lr)

    def get_lr(self):
        t, ti = self.last_epoch, self.T_0
        while t >= ti:
            t -= ti
            ti *= self.T_mult
        return self.eta_min + (self.base_lr - self.eta_min) * (1 + math.cos(math.pi * t / ti)) / 2


def save_checkpoint(model, optimizer, epoch, save_dir, is_best=False):
    """latest_model.pth every call, best_model.pth when is_best, with the
    reference's three keys.  'model_state_dict' loads into the reference model
    unchanged; 'optimizer_state_dict' is upr.optim.Adam's own format (step, the
    flat moment buffers m and v, param_groups), not torch.optim.Adam's."""
    os.makedirs(save_dir, exist_ok=True)
    checkpoint = {
        'epoch': epoch,
        'model_state_dict': {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
        'optimizer_state_dict': {k: (v.detach().cpu() if torch.is_tensor(v) else v)
                                 for k, v in optimizer.state_dict().items()},
    }
    if is_best:
        best_path = os.path.join(save_dir, 'best_model.pth')
        torch.save(checkpoint, best_path)
        print(f"Saved best model: {best_path}")
    latest_path = os.path.join(save_dir, 'latest_model.pth')
    torch.save(checkpoint, latest_path)
    print(f"Saved latest model: {latest_path}")


def load_checkpoint(model, optimizer, checkpoint_path, map_location='cpu'):
    """-> the epoch to resume from (saved epoch + 1).  The file is read with
    map_location (the values are then copied into the model's / optimizer's own
    buffers, wherever they live)."""
    if not os.path.exists(checkpoint_path):
        raise FileNotFoundError(f"Checkpoint not found: {checkpoint_path}")
    checkpoint = torch.load(checkpoint_path, map_location=map_location, weights_only=True)
    model.load_state_dict(checkpoint['model_state_dict'])
    optimizer.load_state_dict(checkpoint['optimizer_state_dict'])
    print(f"Loaded checkpoint from epoch {checkpoint['epoch']}")
    return checkpoint['epoch'] + 1


def _summary_writer(log_dir):
    """TensorBoard's SummaryWriter when tensorboard imports, else None."""
    try:
        import tensorboard  # noqa: F401
        from torch.utils.tensorboard import SummaryWriter
    except Exception:
        return None
    return SummaryWriter(log_dir)


def save_loss_curves(loss_history, save_dir):
    """plots/<key>_curve.png and plots/combined_loss_curves.png (reference :520-568) when matplotlib imports."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except Exception:
        print("matplotlib is not installed: loss curves not drawn (results.csv has the numbers)")
        return False
    plot_dir = os.path.join(save_dir, 'plots')
    os.makedirs(plot_dir, exist_ok=True)
    curves = {k: v for k, v in loss_history.items() if v}
    for key, values in curves.items():
        plt.figure(figsize=(10, 6))
        plt.plot(values)
        plt.title(f'{key.capitalize()} Loss Curve')
        _finish_plot(plt, os.path.join(plot_dir, f'{key}_curve.png'))
    plt.figure(figsize=(12, 8))
    for key, values in curves.items():
        if key != 'total':  # the total would flatten the others
            plt.plot(values, label=key.capitalize())
    plt.title('Training Loss Curves')
    plt.legend()
    _finish_plot(plt, os.path.join(plot_dir, 'combined_loss_curves.png'))
    return True


def _finish_plot(plt, path):
    plt.xlabel('Epoch')
    plt.ylabel('Loss')
    plt.grid(True)
    plt.tight_layout()
    plt.savefig(path)
    plt.close()


def save_results_to_csv(loss_history, save_dir, val_history=None):
    """results.csv: one row per epoch, columns epoch + the loss keys (reference :571-600).
    val_history (column -> one entry per epoch, None where the epoch was not
    validated) appends its columns after them, with empty cells for None."""
    os.makedirs(save_dir, exist_ok=True)
    csv_path = os.path.join(save_dir, 'results.csv')
    keys = list(loss_history)
    vkeys = list(val_history) if val_history else []
    with open(csv_path, 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['epoch'] + keys + vkeys)
        for epoch in range(max((len(v) for v in loss_history.values()), default=0)):
            row = [epoch] + [loss_history[k][epoch] if epoch < len(loss_history[k]) else '' for k in keys]
            for k in vkeys:
                v = val_history[k][epoch] if epoch < len(val_history[k]) else None
                row.append('' if v is None else v)
            w.writerow(row)
    print(f"Saved results to CSV: {csv_path}")
    return csv_path


# ---- validation on held-out images (an addition: the reference's README names --val_data_path,
# its parser has no such flag) ----------------------------------------------------------------
BEST_BY = ('train_total', 'val_total', 'val_psnr', 'val_ssim', 'val_loe')
BEST_BY_PAIRED = ('val_psnr', 'val_ssim')  # need the ground truth; higher is better


def val_columns(paired):
    """The keys of validate()'s dict = the val_* columns of results.csv, in order:
    val_total and the other six loss keys, calculate_metrics' names, val_loe."""
    from utils.utils import metric_names
    return [f'val_{k}' for k in LOSS_KEYS] + [f'val_{n}' for n in metric_names(paired)] + ['val_loe']


def check_best_by(best_by, has_val, has_reference):
    """The rules of --best_by: a val_* choice needs --val_dir, val_psnr and val_ssim also --val_reference_dir."""
    if best_by not in BEST_BY:
        raise ValueError(f"best_by must be one of {BEST_BY}, got {best_by!r}")
    if best_by.startswith('val_') and not has_val:
        raise ValueError(f"--best_by {best_by} needs --val_dir")
    if best_by in BEST_BY_PAIRED and not has_reference:
        raise ValueError(f"--best_by {best_by} needs --val_reference_dir")


def paired_weights(train_reference_dir, weight_rec=None, weight_ssim=None):
    """The rules of --weight_rec / --weight_ssim -> (weight_rec, weight_ssim): both
    default to 1.0 with --train_reference_dir; without it they are unused (0, 0)
    and an explicit value is an error."""
    if train_reference_dir is None:
        given = [n for n, v in (('--weight_rec', weight_rec), ('--weight_ssim', weight_ssim)) if v is not None]
        if given:
            raise ValueError(f"{' and '.join(given)} need{'s' if len(given) == 1 else ''} --train_reference_dir")
        return 0.0, 0.0
    return (1.0 if weight_rec is None else float(weight_rec)), (1.0 if weight_ssim is None else float(weight_ssim))


class BestTracker:
    """Which epoch is the best so far and how long since (best_model.pth, --patience).
    update(train_total, val) -> True (a new best), False (no improvement: the
    patience counter advanced) or None (a val_* choice on an epoch that was not
    validated: neither).  val_psnr and val_ssim are better when higher, the others when lower."""

    def __init__(self, best_by='train_total'):
        self.best_by = best_by
        self.higher = best_by in BEST_BY_PAIRED
        self.best = -float('inf') if self.higher else float('inf')
        self.counter = 0

    def update(self, train_total, val=None):
        if self.best_by == 'train_total':
            v = train_total
        elif val is None:
            return None
        else:
            v = val[self.best_by]
        if (v > self.best) if self.higher else (v < self.best):
            self.best, self.counter = v, 0
            return True
        self.counter += 1
        return False


def make_val_loaders(val_dir, reference_dir=None, image_size=640, batch_size=8, num_workers=4, device=None):
    """(loader, reference_loader or None) over the held-out images: LowLightDataset
    without augmentation (every image letterboxed to image_size), in file order,
    the short last batch kept.  The ground truth of NAME.ext is the file of
    reference_dir with stem NAME, loaded the same way."""
    from datasets.dataset import DeviceLoader, LowLightDataset, match_by_stem

    def loader(ds):
        ds.device = device
        # seed 0: the (unused) draws would come from a generator of the loader's own, never the global `random`
        return DeviceLoader(ds, batch_size=batch_size, shuffle=False, num_workers=num_workers, drop_last=False,
                            device=device, seed=0)

    ds = LowLightDataset(val_dir, image_size=image_size, augment=False, advanced_augment=False)
    if reference_dir is None:
        return loader(ds), None
    ref = LowLightDataset(reference_dir, image_size=image_size, augment=False, advanced_augment=False)
    ref.image_files = match_by_stem(ds.image_files, ref.image_files, reference_dir)
    return loader(ds), loader(ref)


def validate(model, loader, criterion, device, reference_loader=None, loe_size=50, on_batch=None):
    """One pass over held-out images: the eval-mode forward in fp32 under
    no_grad (the inference executor, whatever --use_amp says), TotalLoss forward
    only (criterion.evaluate: constructor weights, no DWA, no history),
    batch_metrics against the ground truth of reference_loader when given, and
    batch_loe against the input.  Per-image values are summed on the device in
    fp64 (a batch's loss terms weighted by its image count); one device-to-host
    copy at the end.  Returns {val_columns(paired)[i]: mean over the images}.
    on_batch(first_index, low, enh, illu), when given, sees every batch (the
    sample panels).  The run is left as found: no parameter, buffer, optimiser,
    scaler, loss history or `random` state changes; model.training is restored."""
    from upr.loss_engine import TERM_ORDER
    from utils.utils import batch_loe, batch_metrics, metric_names
    paired = reference_loader is not None
    names = metric_names(paired)
    order = [TERM_ORDER.index(k) for k in LOSS_KEYS]
    was_training = model.training
    model.eval()
    sums, n = None, 0
    try:
        with torch.no_grad(), torch.autocast("cuda", enabled=False):
            refs = iter(reference_loader) if paired else None
            for low in loader:
                low = low.to(device, torch.float32)
                gt = None
                if paired:
                    gt = next(refs).to(device, torch.float32)
                    if gt.shape != low.shape:
                        files = loader.dataset.image_files[n:n + low.shape[0]]
                        rfiles = reference_loader.dataset.image_files[n:n + low.shape[0]]
                        raise ValueError(f"ground truth {rfiles} letterboxes to {tuple(gt.shape[2:])}, "
                                         f"{files} to {tuple(low.shape[2:])}")
                enh, refl, illu = model(low)
                terms = criterion.evaluate(low, enh, illu, refl)
                m = batch_metrics(enh, gt)
                b = low.shape[0]
                row = torch.cat([terms[order].double() * b, torch.stack([m[k] for k in names]).sum(dim=1),
                                 batch_loe(low, enh, loe_size).sum().reshape(1)])
                sums = row if sums is None else sums + row
                if on_batch is not None:
                    on_batch(n, low, enh, illu)
                n += b
    finally:
        model.train(was_training)
    if n == 0:
        raise ValueError("validate: the loader gave no images")
    return dict(zip(val_columns(paired), (sums / n).cpu().tolist()))  # the one device-to-host copy


def save_val_samples(sample_dir, files, first, low, enh, illu, k, output_format=None):
    """<sample_dir>/<stem>_comparison.<ext> for the images of this batch among the
    first k of the validation set: the [input | enhanced | illumination] panel
    of enhancers.simple_enhance.create_comparison (the reference's
    save_sample_visualizations, :399-517, without torchvision / matplotlib)."""
    from enhancers.simple_enhance import create_comparison
    fmt = dict(output_format or {})
    ext = fmt.get('image_format', 'png')
    os.makedirs(sample_dir, exist_ok=True)
    for i in range(max(0, min(low.shape[0], k - first))):
        stem = os.path.splitext(os.path.basename(files[first + i]))[0]
        create_comparison(low[i:i + 1], enh[i:i + 1], os.path.join(sample_dir, f"{stem}_comparison.{ext}"),
                          illu_map=illu[i:i + 1], **fmt)


def _output_format(args):
    return dict(png_encoder=getattr(args, 'png_encoder', 'host'), image_format=getattr(args, 'image_format', 'png'),
                jpeg_quality=getattr(args, 'jpeg_quality', 95), jpeg_subsampling=getattr(args, 'jpeg_subsampling', '444'),
                jpeg_optimize=getattr(args, 'jpeg_optimize', False),
                jpeg_gray_maps=getattr(args, 'jpeg_gray_maps', False))


def train(args):
    """The reference's train(args) (trainers/train.py:189-396) on the HIP step
    and the device data path.  Differences: the schedulers are this module's
    (closed forms; a resumed run continues the schedule at its epoch instead of
    restarting it), TensorBoard and the matplotlib curves are used when they
    import, save_sample_visualizations is replaced by the validation pass's
    panels, and the rows of results.csv are the epochs this call ran.
    With --val_dir, validate() runs after every --val_freq-th epoch and after the
    last one: its numbers are printed, logged as Val/<name>, appended to
    results.csv as val_* columns, and --best_by may pick best_model.pth and drive
    --patience by one of them.  Returns the loss history."""
    from datasets.dataset import get_train_dataloader
    from losses.loss import TotalLoss
    from models.model import MultiScaleUP_Retinex

    val_dir, val_ref_dir = getattr(args, 'val_dir', None), getattr(args, 'val_reference_dir', None)
    best_by = getattr(args, 'best_by', 'train_total')
    check_best_by(best_by, val_dir is not None, val_ref_dir is not None)
    if not torch.cuda.is_available():
        raise RuntimeError("--mode train runs on ROCm devices only (no CPU fallback)")
    dev = getattr(args, 'device', None)
    device = torch.device(dev if dev and str(dev) != 'cpu' else 'cuda')
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    print(f"Using device: {device}")
    seed = getattr(args, 'seed', None)
    if seed is not None:
        torch.manual_seed(seed)
    use_preact, use_aspp = getattr(args, 'use_preact', False), getattr(args, 'use_aspp', False)
    model = MultiScaleUP_Retinex(use_preact=use_preact, use_aspp=use_aspp).to(device)
    print(f"Number of parameters: {sum(p.numel() for p in model.parameters() if p.requires_grad):,}")
    use_freq_loss, adaptive_weights = getattr(args, 'use_freq_loss', False), getattr(args, 'adaptive_weights', False)
    train_ref_dir = getattr(args, 'train_reference_dir', None)
    weight_rec, weight_ssim = paired_weights(train_ref_dir, getattr(args, 'weight_rec', None),
                                             getattr(args, 'weight_ssim', None))
    criterion = TotalLoss(weight_exp=getattr(args, 'weight_exp', 10.0), weight_smooth=getattr(args, 'weight_smooth', 1.0),
                          weight_col=getattr(args, 'weight_col', 0.5), weight_spa=getattr(args, 'weight_spa', 1.0),
                          weight_decouple=getattr(args, 'weight_decouple', 0.1),
                          weight_perceptual=getattr(args, 'weight_perceptual', 1.0),
                          weight_freq=getattr(args, 'weight_freq', 0.5), use_freq_loss=use_freq_loss,
                          adaptive_weights=adaptive_weights, weight_rec=weight_rec, weight_ssim=weight_ssim,
                          rec_eps=getattr(args, 'rec_eps', 1e-3)).to(device)
    print(f"Loss: frequency term {'on' if use_freq_loss else 'off'}, adaptive weights "
          f"{'on' if adaptive_weights else 'off'}" +
          (f", paired terms against '{train_ref_dir}': reconstruction x {weight_rec:g}, ssim_loss x {weight_ssim:g}"
           if train_ref_dir is not None else ""))
    optimizer = make_optimizer(model, lr=args.lr, weight_decay=args.weight_decay)
    use_amp = bool(getattr(args, 'use_amp', False))
    scaler = GradScaler() if use_amp else None
    if use_amp:
        print("Mixed precision training enabled (AMP)")
    patience = getattr(args, 'patience', 20)
    start_epoch = 0
    if getattr(args, 'resume', None):
        start_epoch = load_checkpoint(model, optimizer, args.resume, map_location='cpu')
    if getattr(args, 'use_cosine_scheduler', False):
        scheduler = CosineAnnealingWarmRestarts(optimizer, T_0=10, T_mult=2, eta_min=1e-6, last_epoch=start_epoch,
                                                base_lr=args.lr)
    else:
        scheduler = StepLR(optimizer, step_size=args.lr_decay_step, gamma=args.lr_decay_gamma,
                           last_epoch=start_epoch, base_lr=args.lr)
    advanced_augment = getattr(args, 'advanced_augment', False)
    train_loader = get_train_dataloader(image_dir=args.train_dir, batch_size=args.batch_size,
                                        image_size=args.image_size, num_workers=args.num_workers, shuffle=True,
                                        advanced_augment=advanced_augment, device=device, seed=seed,
                                        reference_dir=train_ref_dir)
    print(f"Number of training batches: {len(train_loader)}")
    if len(train_loader) == 0:
        print(f"No training batches: {len(train_loader.dataset)} samples, batch_size={args.batch_size}")
        return None
    val_loader = val_ref_loader = None
    if val_dir is not None:
        val_loader, val_ref_loader = make_val_loaders(
            val_dir, val_ref_dir, image_size=args.image_size,
            batch_size=getattr(args, 'val_batch_size', None) or args.batch_size, num_workers=args.num_workers,
            device=device)
        print(f"Validation: {len(val_loader.dataset)} images in {len(val_loader)} batches, best model by {best_by}")
    val_freq, val_samples = getattr(args, 'val_freq', 1), getattr(args, 'val_samples', 4)
    save_freq, loe_size = getattr(args, 'save_freq', 10), getattr(args, 'loe_size', 50)
    val_history = {k: [] for k in val_columns(val_ref_loader is not None)} if val_loader is not None else None

    def run_validation(epoch, samples):
        """validate() -> its dict, printed and logged; samples: also write this epoch's panels."""
        on_batch = None
        if samples:
            sample_dir = os.path.join(args.save_dir, 'samples', f'epoch_{epoch + 1:04d}')
            files, fmt = val_loader.dataset.image_files, _output_format(args)

            def on_batch(first, low, enh, illu):
                save_val_samples(sample_dir, files, first, low, enh, illu, val_samples, fmt)
        t0 = time.time()
        val_loader.set_epoch(0)
        if val_ref_loader is not None:
            val_ref_loader.set_epoch(0)
        val = validate(model, val_loader, criterion, device, reference_loader=val_ref_loader, loe_size=loe_size,
                       on_batch=on_batch)
        print(f"  Validation: {time.time() - t0:.2f}s, " + ", ".join(f"{k} {v:.6f}" for k, v in val.items()))
        if writer is not None:
            for k, v in val.items():
                writer.add_scalar(f"Val/{k[len('val_'):]}", v, epoch)
        return val

    writer = _summary_writer(os.path.join(args.save_dir, 'logs', datetime.now().strftime('%Y%m%d_%H%M%S')))
    loss_keys = LOSS_KEYS + (PAIRED_KEYS if train_ref_dir is not None else ())
    loss_history = {k: [] for k in loss_keys}
    tracker = BestTracker(best_by)
    for epoch in range(start_epoch, args.num_epochs):
        train_loader.set_epoch(epoch)
        avg = train_one_epoch(model, train_loader, criterion, optimizer, device, epoch, writer, scaler=scaler,
                              use_amp=use_amp)
        scheduler.step()
        current_lr = optimizer.param_groups[0]['lr']
        for k in loss_keys:
            loss_history[k].append(float(avg[k]))
        print(f"\nEpoch {epoch}: {avg['_epoch_seconds']:.2f}s, lr {current_lr:.6g}, " +
              ", ".join(f"{k} {loss_history[k][-1]:.6f}" for k in loss_keys))
        if writer is not None:
            writer.add_scalar('Learning_Rate', current_lr, epoch)
            for k in loss_keys:
                writer.add_scalar(f'Epoch_Loss/{k}', loss_history[k][-1], epoch)
        val, sampled = None, False
        if val_loader is not None:
            last = epoch == args.num_epochs - 1
            if (epoch + 1) % val_freq == 0 or last:
                sampled = val_samples > 0 and ((epoch + 1) % save_freq == 0 or last)
                val = run_validation(epoch, sampled)
        is_best = tracker.update(loss_history['total'][-1], val)
        if is_best:
            print(f"  New best {'loss' if best_by == 'train_total' else best_by}: {tracker.best:.6f}")
        elif is_best is None:
            print(f"  Not validated: best {best_by} and patience unchanged")
        else:
            print(f"  Patience: {tracker.counter}/{patience}")
        stop = tracker.counter >= patience
        if stop and val_loader is not None and (val is None or (val_samples > 0 and not sampled)):
            # early stopping makes this the last epoch run: it is validated, and its panels written
            again = run_validation(epoch, val_samples > 0)
            val = again if val is None else val
        if val_history is not None:
            for k in val_history:
                val_history[k].append(None if val is None else val[k])
        save_checkpoint(model, optimizer, epoch, args.save_dir, bool(is_best))
        if stop:
            print(f"Early stopping after {epoch + 1} epochs, best loss {tracker.best:.6f}")
            break
    best_loss = tracker.best
    if writer is not None:
        writer.close()
    save_loss_curves(loss_history, args.save_dir)
    save_results_to_csv(loss_history, args.save_dir, val_history)
    print(f"Training completed. Best loss: {best_loss:.6f}. Models saved in: {args.save_dir}")
    return loss_history
