"""The flat parameter / gradient buffers of clip_grad_norm_ and Adam (csrc/train_optim.hip)."""
import torch

from .._dev import F32


class FlatParams:
    """All trainable parameters of a module in one flat device buffer (and the
    gradients in another); each nn.Parameter's .data / .grad become views.
    Order = module.named_parameters() (the reference optimiser's order)."""

    def __init__(self, module):
        params = list(module.named_parameters()) if hasattr(module, "named_parameters") else \
            [(str(i), p) for i, p in enumerate(module)]
        dev = params[0][1].device
        if dev.type != "cuda":
            raise RuntimeError("HIP training needs the parameters on a ROCm device (model.to('cuda'))")
        align = 16  # 64-byte aligned tensors (the conv kernels' vector loads of bias / weights)
        n = sum((p.numel() + align - 1) // align * align for _, p in params)
        self.numel = n
        self.flat = torch.zeros((n,), dtype=F32, device=dev)
        self.grad = torch.zeros((n,), dtype=F32, device=dev)
        self.offsets = {}
        off = 0
        for name, p in params:
            k = p.numel()
            self.flat[off:off + k].view(p.shape).copy_(p.data)   # one-time device copy (plumbing)
            p.data = self.flat[off:off + k].view(p.shape)
            p._upr_flat = self
            self.offsets[name] = (off, k)
            off += (k + align - 1) // align * align
        self.params = dict(params)
        self.attach_grads()

    def attach_grads(self):
        """(Re)point every .grad at its slice of the flat gradient buffer;
        returns True if any had been detached (zero_grad(set_to_none=True))."""
        detached = False
        for name, p in self.params.items():
            off, k = self.offsets[name]
            g = p.grad
            if g is None or g.data_ptr() != self.grad.data_ptr() + 4 * off:
                detached = True
                p.grad = self.grad[off:off + k].view(p.shape)
        return detached

