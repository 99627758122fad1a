"""UP-Retinex losses (drop-in for the reference losses/loss.py).

Same classes, constructor arguments and forward signatures; the arithmetic
runs on the gfx950 kernels of upr/loss_engine.py (include/upr_train.h).
`TotalLoss.forward` returns `(total_loss, loss_dict)` like the reference
(:656-753); `total_loss.backward()` sends the loss gradients into the model's
HIP backward.  The individual term classes are differentiable modules too
(the engine with weight 1 on their term), with the reference's constructor
arguments (patch_size, base_target_exposure, lambda_val, alpha, weight_high,
weight_low) passed to the kernels (include/upr_train.h UprLossParams).

Differences, all forced by the environment and recorded in DESIGN.md:
  * PerceptualLoss loads torchvision's pretrained VGG-19 in the reference
    (:195, a download).  Here `vgg_weights=` takes a features state_dict
    (e.g. a local copy of torchvision's vgg19 weights); without one the VGG is
    PyTorch-default-initialised under `vgg_seed` (1234, the seed the parity
    fixtures use).
  * adaptive_weights=True (DWA, :755-798) keeps the reference's host loss
    history; texture_method 'tv' and 'edge_density' both run on the device;
    use_dynamic_smooth_weight=False uses weight_smooth as is.
"""
import threading

import torch
import torch.nn as nn

from upr import loss_engine as E
from upr.autograd import loss_forward, paired_forward

_VGG_SEED = 1234


def _require(t, name):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError(f"{name}: UP-Retinex losses run on ROCm devices only (got "
                           f"{getattr(t, 'device', type(t))})")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: float32 tensors expected, got {t.dtype}")


def _features(vgg_weights, vgg_seed):
    f = E.vgg19_features(seed=vgg_seed)
    if vgg_weights is not None:
        f.load_state_dict(vgg_weights)
    for p in f.parameters():
        p.requires_grad = False
    return f


class _EngineHolder(nn.Module):
    _weights = None
    _params = None
    use_freq_loss = True
    texture_method = "tv"

    def _engine(self, dev):
        eng = self.__dict__.get("_eng")
        if eng is None or eng[0] != dev:
            feats = self.features.to(dev) if hasattr(self, "features") else None
            eng = (dev, E.TotalLossEngine(feats, weights=self._weights, use_freq_loss=self.use_freq_loss,
                                          texture_method=self.texture_method, params=self._params))
            self.__dict__["_eng"] = eng
        return eng[1]


class _Term(_EngineHolder):
    """One loss term as its own differentiable module: the loss engine with
    weight 1 on this term and 0 elsewhere (the smoothness weight fixed, not
    dynamic), so the returned 0-dim tensor IS the term and its backward is the
    term's gradient w.r.t. the module's differentiable inputs."""

    _term = None

    def _setup(self, **params):
        w = {k: 0.0 for k in E.WEIGHTS}
        w[self._term] = 1.0
        self._weights = w
        p = dict(E.PARAMS)
        p.update(params)
        p["dynamic_smooth"] = False
        self._params = p
        self.use_freq_loss = self._term == "frequency"

    def _eval(self, low, enh, illu, refl):
        for t, n in ((low, "img_low"), (enh, "img_enhanced"), (illu, "illu_map"), (refl, "reflectance")):
            _require(t, n)
        total, _ = loss_forward(self._engine(enh.device), low.contiguous(), enh.contiguous(), illu.contiguous(),
                                refl.contiguous())
        return total


def _dummy_illu(x):
    return x[:, :1].contiguous()


class AdaptiveExposureLoss(_Term):
    """L_exp (reference :12-58): mean |avgpool_ps(gray(R)) - (b + (0.8 - b)(1 - mean gray(S)))|."""

    _term = "exposure"

    def __init__(self, patch_size=16, base_target_exposure=0.6):
        super().__init__()
        if int(patch_size) != patch_size or patch_size < 1:
            raise ValueError(f"patch_size must be a positive integer, got {patch_size}")
        self.patch_size, self.base_target_exposure = patch_size, base_target_exposure
        self._setup(patch=int(patch_size), base_exposure=float(base_target_exposure))

    def forward(self, img_enhanced, img_low):
        return self._eval(img_low, img_enhanced, _dummy_illu(img_enhanced), img_enhanced)


class EdgeAwareSmoothnessLoss(_Term):
    """L_smooth (reference :61-176): exp(-lambda |grad S|) x (1 + alpha x row / column edge means) x |grad I|."""

    _term = "smoothness"

    def __init__(self, lambda_val=10.0, alpha=1.0):
        super().__init__()
        self.lambda_val, self.alpha = lambda_val, alpha
        self._setup(smooth_lambda=float(lambda_val), smooth_alpha=float(alpha))

    def forward(self, illu_map, img_low):
        # illu_map [B,1,H,W] (the model's) or [B,3,H,W] (the reference self-test's, loss.py:806-819):
        # the mean runs over every illumination plane (:171-172)
        if illu_map.dim() != 4 or illu_map.shape[1] not in (1, 3):
            raise NotImplementedError("device smoothness loss: illumination [B,1,H,W] or [B,3,H,W]")
        return self._eval(img_low, img_low, illu_map, img_low)


class ColorLoss(_Term):
    """L_col gray-world (reference :337-371)."""

    _term = "color"

    def __init__(self):
        super().__init__()
        self._setup()

    def forward(self, img_enhanced):
        # img_low is a placeholder here (the term does not read it)
        return self._eval(img_enhanced.detach(), img_enhanced, _dummy_illu(img_enhanced), img_enhanced)


class SpatialConsistencyLoss(_Term):
    """L_spa (reference :374-427)."""

    _term = "spatial"

    def __init__(self):
        super().__init__()
        self._setup()

    def forward(self, img_enhanced, img_low):
        return self._eval(img_low, img_enhanced, _dummy_illu(img_enhanced), img_enhanced)


class IlluminationReflectanceDecouplingLoss(_Term):
    """L_decouple (reference :258-334): ||cov||_F^2 + lambda x mse(means), for the
    model's C_illu = 1 (the expanded, uncentred illumination against the
    centred reflectance, :308-312; channel-mean means, :326-329) and for
    C_illu = C_refl = 3 (the centred 3x3 covariance, :302-304; per-channel
    means, :323-324).  Other channel counts (:313-317) are refused."""

    _term = "decouple"

    def __init__(self, lambda_val=0.1):
        super().__init__()
        self.lambda_val = lambda_val
        self._setup(decouple_lambda=float(lambda_val))

    def forward(self, illu_map, reflectance):
        if illu_map.shape[1] not in (1, 3) or reflectance.shape[1] != 3:
            raise NotImplementedError("device decoupling loss: illumination [B,1,H,W] or [B,3,H,W], "
                                      "reflectance [B,3,H,W]")
        return self._eval(reflectance.detach(), reflectance, illu_map, reflectance)  # img_low: placeholder


class PerceptualLoss(_Term):
    """L_perceptual (reference :179-255): VGG-19 slices to pool3, summed MSEs."""

    _term = "perceptual"

    def __init__(self, device='cpu', vgg_weights=None, vgg_seed=_VGG_SEED):
        super().__init__()
        self.features = _features(vgg_weights, vgg_seed)
        self.register_buffer('mean', torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1))
        self.register_buffer('std', torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1))
        self._setup()

    def forward(self, img_enhanced, img_low):
        return self._eval(img_low, img_enhanced, _dummy_illu(img_enhanced), img_enhanced)


class FrequencyLoss(_Term):
    """L_freq (reference :430-520): weighted MSE of FFT magnitudes (weight_high
    outside radius min(H, W)/4 of the unshifted centre, weight_low inside)."""

    _term = "frequency"

    def __init__(self, weight_high=1.0, weight_low=0.5):
        super().__init__()
        self.weight_high, self.weight_low = weight_high, weight_low
        self._setup(freq_high=float(weight_high), freq_low=float(weight_low))

    def forward(self, img_enhanced, img_low):
        return self._eval(img_low, img_enhanced, _dummy_illu(img_enhanced), img_enhanced)


class _PairedTerm(nn.Module):
    """One paired term against a ground truth as its own differentiable module
    (an addition: the reference trains without labels).  Any H, W >= 1; the
    gradient goes to img_enhanced only (a target that requires grad is refused)."""

    _index = None
    eps = E.REC_EPS

    def forward(self, img_enhanced, target):
        _require(img_enhanced, "img_enhanced")
        _require(target, "target")
        return paired_forward(img_enhanced.contiguous(), target.contiguous(), self._index, float(self.eps))


class ReconstructionLoss(_PairedTerm):
    """Charbonnier: mean sqrt((img_enhanced - target)^2 + eps^2)."""

    _index = 0

    def __init__(self, eps=1e-3):
        super().__init__()
        self.eps = eps


class SSIMLoss(_PairedTerm):
    """1 - mean SSIM, the SSIM of utils.utils.calculate_ssim (11 x 11 box window
    over a zero border, per channel, every position)."""

    _index = 1


class TotalLoss(_EngineHolder):
    """TotalLoss (reference :586-753).  Additions: weight_rec / weight_ssim /
    rec_eps and criterion(..., target=): with a ground truth the Charbonnier and
    1 - SSIM terms against it join the total under those two weights (outside
    DWA) and the loss_dict as 'reconstruction' and 'ssim_loss'."""

    def __init__(self, weight_exp=10.0, weight_smooth=1.0, weight_col=0.5, weight_spa=1.0, weight_decouple=0.1,
                 weight_perceptual=1.0, weight_freq=0.5, use_freq_loss=True, adaptive_weights=False,
                 use_dynamic_smooth_weight=True, texture_method='tv', vgg_weights=None, vgg_seed=_VGG_SEED,
                 weight_rec=0.0, weight_ssim=0.0, rec_eps=1e-3):
        super().__init__()
        self.weight_rec, self.weight_ssim, self.rec_eps = float(weight_rec), float(weight_ssim), float(rec_eps)
        if texture_method not in E.TEXTURE:
            raise ValueError(f"不支持的纹理复杂度计算方法: {texture_method}")
        self.features = _features(vgg_weights, vgg_seed)
        self.use_freq_loss = use_freq_loss
        self.adaptive_weights = adaptive_weights
        self.use_dynamic_smooth_weight = use_dynamic_smooth_weight
        self.texture_method = texture_method
        self._weights = dict(exposure=weight_exp, smoothness=weight_smooth, color=weight_col, spatial=weight_spa,
                             decouple=weight_decouple, perceptual=weight_perceptual, frequency=weight_freq)
        # TotalLoss builds its terms with their default arguments (loss.py:620-626)
        self._params = dict(E.PARAMS, dynamic_smooth=bool(use_dynamic_smooth_weight))
        if adaptive_weights:
            self.loss_history = {k: [] for k in _DWA_KEYS}

    def __call__(self, *args, target=None, **kwargs):
        """criterion(img_low, img_enhanced, illu_map, reflectance=None, epoch=0, target=None).  forward keeps
        the reference's five parameters; a ground truth is a keyword of the call and takes the paired path."""
        if target is None:
            return super().__call__(*args, **kwargs)
        return self._forward(*args, target=target, **kwargs)

    def forward(self, img_low, img_enhanced, illu_map, reflectance=None, epoch=0):
        return self._forward(img_low, img_enhanced, illu_map, reflectance, epoch)

    def _forward(self, img_low, img_enhanced, illu_map, reflectance=None, epoch=0, target=None):
        no_refl = reflectance is None
        for t, n in ((img_low, "img_low"), (img_enhanced, "img_enhanced"), (illu_map, "illu_map"),
                     (reflectance, "reflectance"), (target, "target")):
            if t is not None:
                _require(t, n)
        if no_refl:
            # loss.py:678-682: no reflectance -> the decoupling term is 0.  The
            # kernels still take a [B,3,H,W] operand: the enhanced image stands
            # in (weight 0: no contribution to the total or any gradient), and
            # the term is reported as exactly 0
            reflectance = img_enhanced.detach()
        eng = self._engine(img_enhanced.device)
        # weights of this step (loss.py:690-702): DWA from the history after epoch 1
        eng.w = self._compute_adaptive_weights() if self.adaptive_weights and epoch > 1 else dict(self._weights)
        if no_refl:
            eng.w["decouple"] = 0.0
        eng.zero_decouple = no_refl
        eng.w_rec, eng.w_ssim, eng.rec_eps = self.weight_rec, self.weight_ssim, self.rec_eps
        total, terms = loss_forward(eng, img_low.contiguous(), img_enhanced, illu_map, reflectance,
                                    target=None if target is None else target.contiguous())
        d = E.terms_dict(terms, lazy=_defer_readback() and not self.adaptive_weights)
        if self.adaptive_weights:
            for k in _DWA_KEYS:
                self.loss_history[k].append(d[k])
        return total, d

    def evaluate(self, img_low, img_enhanced, illu_map, reflectance=None):
        """Forward only, for held-out data (trainers.train.validate): the terms
        under the constructor weights -- no DWA, nothing appended to
        loss_history, no autograd graph, no host read-back.  Returns the device
        float32 tensor of the engine's scalars in upr.loss_engine.TERM_ORDER
        (exposure .. frequency, total at 7), the dynamic smooth weight at 8."""
        no_refl = reflectance is None
        for t, n in ((img_low, "img_low"), (img_enhanced, "img_enhanced"), (illu_map, "illu_map"),
                     (reflectance, "reflectance")):
            if t is not None:
                _require(t, n)
        if no_refl:
            reflectance = img_enhanced
        eng = self._engine(img_enhanced.device)
        eng.w = dict(self._weights)
        if no_refl:
            eng.w["decouple"] = 0.0
        eng.zero_decouple = no_refl
        with torch.no_grad():
            _, terms = loss_forward(eng, img_low.contiguous(), img_enhanced.contiguous(), illu_map.contiguous(),
                                    reflectance.contiguous())
        return terms

    def _compute_adaptive_weights(self):
        """Dynamic Weight Average (loss.py:755-798): w_k = (L_k[-1] / L_k[-2]) / T
        (T = 2, ratio 1 when L_k[-2] <= 1e-8; the constructor weight while a
        term has < 2 entries), renormalised to sum to the number of terms.  The
        smoothness weight is then replaced by the dynamic smooth weight."""
        return dwa_weights(self.loss_history, self._weights)


_DWA_KEYS = ("exposure", "smoothness", "color", "spatial", "decouple", "perceptual", "frequency")

# set by trainers.train.train_step around its criterion call: the loss_dict's
# host read-back is deferred until the step's backward and optimizer work is
# queued (the step returns it materialised), instead of draining the device
# between the forward and the backward as the reference's .item()s do.
# Per thread: another thread's criterion call never sees this one's switch.
_DEFER_READBACK = threading.local()


def _defer_readback():
    return getattr(_DEFER_READBACK, "on", False)


class deferred_readback:
    def __enter__(self):
        self._prev = _defer_readback()
        _DEFER_READBACK.on = True

    def __exit__(self, *exc):
        _DEFER_READBACK.on = self._prev


def dwa_weights(history, defaults, temperature=2.0):
    """The weight rule of TotalLoss._compute_adaptive_weights (loss.py:755-798)
    over host loss histories (python floats, as the reference's .item()s)."""
    w = {}
    for k in history:
        h = history[k]
        if len(h) >= 2:
            ratio = h[-1] / h[-2] if h[-2] > 1e-8 else 1.0
            w[k] = ratio / temperature
        else:
            w[k] = defaults.get(k, 1.0)
    tot = sum(w.values())
    if w and tot > 0:
        n = len(w)
        w = {k: n * v / tot for k, v in w.items()}
    return w


def calculate_texture_complexity(img, method='tv'):
    """Texture complexity per image (reference losses/loss.py:523-583) on the
    device (upr_t_texture_complexity): 'tv' = mean |horizontal difference| +
    mean |vertical difference| over C, H, W; 'edge_density' = the share of
    pixels whose reflect-padded Sobel magnitude of the channel-mean gray
    exceeds 1.5x its image mean.  img [B,C,H,W] float32 on a ROCm device ->
    [B] float32.  TotalLoss uses it for the dynamic smoothness weight without
    gradient, and so does this function (no autograd history)."""
    if method not in E.TEXTURE:
        raise ValueError(f"不支持的纹理复杂度计算方法: {method}")
    _require(img, "calculate_texture_complexity")
    if img.dim() != 4:
        raise RuntimeError(f"calculate_texture_complexity: expected [B,C,H,W], got {tuple(img.shape)}")
    return E.texture_complexity(img.detach().contiguous(), E.TEXTURE[method])