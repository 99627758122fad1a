"""Training engine: explicit forward + backward of MultiScaleUP_Retinex on the
gfx950 kernels of include/upr_train.h (+ the inference conv kernels).

Reference: trainers/train.py:63-103 runs `model(img_low)` in train mode,
`criterion(...)` (losses/loss.py TotalLoss), `loss.backward()`,
`clip_grad_norm_(1.0)` and `Adam.step()` on PyTorch autograd.  Here the same
step is a fixed graph written out by hand: every layer object owns the
forward kernels of one reference module and the matching backward kernels;
activations the backward needs are kept from the forward.  PyTorch only
allocates device memory (torch.empty) and supplies the stream; there is no
autograd tape and no torch compute.

Layouts: network input / outputs NCHW (the reference's tensors), every
activation NHWC fp32 (`Act`, possibly a channel slice of a concat buffer).
Parameters and their gradients live in ONE flat fp32 buffer each
(`FlatParams`), so clip_grad_norm_ and Adam are single launches.

Modules follow the csrc units: state, act, params, conv, bn, ops, blocks, graph;
device plumbing is upr/_dev.py.
"""
from .act import Act, Concat, Half, nchw_view  # noqa: F401 (re-exports, all of them)
from .blocks import ASPPT, FAMT, IENetT, PreActResBlockT, ResBlockT, UpBlockT
from .bn import BN, chan_sum
from .conv import Conv, ConvT, mfma16, pack_convs
from .graph import UPRetinexTrainGraph
from .ops import add_into, maxpool_into, pointwise, relu_mask
from .params import FlatParams
from .state import _AMP, FP16_ONLY_STORES, autocast_active, profile_begin, profile_end, set_amp
