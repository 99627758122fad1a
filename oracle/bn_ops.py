"""float64 restatement of the BatchNorm training ops and of clip + Adam
(include/upr_train.h, BatchNorm and optimiser sections) on [M, C] numpy arrays.

Plain numpy, no torch in the arithmetic: the op-level GPU tests
(tests/test_gpu_bn_ops.py) measure the kernels against this, and
tests/test_cpu_bn_ops_oracle.py checks it against torch.nn.BatchNorm2d with
autograd and torch.optim.Adam, both in double.
"""
import numpy as np

F64 = np.float64


def _f64(a):
    return None if a is None else np.asarray(a, dtype=F64)


def bn_stats(x, eps):
    """mean, biased variance and 1/sqrt(var + eps) per channel of x[M, C]."""
    x = _f64(x)
    mean = x.mean(axis=0)
    var = ((x - mean) ** 2).mean(axis=0)
    return mean, var, 1.0 / np.sqrt(var + F64(eps))


def bn_running(running_mean, running_var, mean, var, M, momentum):
    """nn.BatchNorm2d's running-statistic update: the unbiased variance
    (var * M / (M - 1); M = 1 keeps var) and momentum."""
    unb = var * M / (M - 1) if M > 1 else var
    mom = F64(momentum)
    return (1.0 - mom) * _f64(running_mean) + mom * mean, (1.0 - mom) * _f64(running_var) + mom * unb


def bn_eval_stats(running_mean, running_var, eps):
    """Eval-mode statistics: mean = running_mean, invstd = 1/sqrt(running_var + eps)."""
    return _f64(running_mean).copy(), 1.0 / np.sqrt(_f64(running_var) + F64(eps))


def bn_affine(x, mean, invstd, gamma, beta):
    """gamma * (x - mean) * invstd + beta (the value whose sign is the ReLU mask)."""
    return _f64(gamma) * ((_f64(x) - _f64(mean)) * _f64(invstd)) + _f64(beta)


def bn_apply(x, mean, invstd, gamma, beta, res=None, res_post=False, relu=False):
    """y = [relu](gamma*(x-mean)*invstd + beta + res_pre) + res_post."""
    v = bn_affine(x, mean, invstd, gamma, beta)
    r = _f64(res)
    if r is not None and not res_post:
        v = v + r
    if relu:
        v = np.maximum(v, 0.0)
    if r is not None and res_post:
        v = v + r
    return v


def bn_bwd(g, x, mean, invstd, gamma, batch_stats=True, mask=None, dx0=None, dgamma0=None, dbeta0=None):
    """BatchNorm backward from g = d(loss)/d(bn output).

    mask (bool [M, C], optional): the consumer ReLU folded in, g counts where
    mask is set.  batch_stats: dx = gamma*invstd*(g - sum(g)/M - xhat*sum(g*xhat)/M);
    otherwise (running statistics are constants) dx = gamma*invstd*g.  dx0
    (optional) is added to dx (an accumulated input gradient); dgamma0 / dbeta0
    are the parameter gradients' previous values (always accumulated).
    Returns dx, dgamma, dbeta, (sum g, sum g*xhat)."""
    g, x = _f64(g), _f64(x)
    if mask is not None:
        g = np.where(np.asarray(mask, dtype=bool), g, 0.0)
    M = x.shape[0]
    xh = (x - _f64(mean)) * _f64(invstd)
    sg, sgx = g.sum(axis=0), (g * xh).sum(axis=0)
    gi = _f64(gamma) * _f64(invstd)
    dx = gi * (g - sg / M - xh * (sgx / M)) if batch_stats else gi * g
    if dx0 is not None:
        dx = dx + _f64(dx0)
    dgamma = sgx + (0.0 if dgamma0 is None else _f64(dgamma0))
    dbeta = sg + (0.0 if dbeta0 is None else _f64(dbeta0))
    return dx, dgamma, dbeta, (sg, sgx)


def chan_sum(g, out0=None):
    """Per-channel sum over the rows of g[M, C] (+ out0 when accumulating)."""
    s = _f64(g).sum(axis=0)
    return s if out0 is None else s + _f64(out0)


def clip_coef(g, max_norm):
    """torch.nn.utils.clip_grad_norm_: (total L2 norm, min(max_norm/(norm+1e-6), 1))."""
    g = _f64(g)
    norm = np.sqrt((g * g).sum())
    return norm, min(F64(max_norm) / (norm + 1e-6), 1.0)


def adam_step(p, g, m, v, step, lr, betas, eps, weight_decay, max_norm=None):
    """One clip_grad_norm_(max_norm) (skipped when max_norm is None) +
    torch.optim.Adam step (L2 decay added to the gradient, bias-corrected
    moments); step counts from 1.  Returns p, m, v, norm (None without clip)."""
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    b1, b2 = F64(betas[0]), F64(betas[1])
    norm = None
    if max_norm is not None:
        norm, coef = clip_coef(g, max_norm)
        g = g * coef
    g = g + F64(weight_decay) * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    p = p - (F64(lr) / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + F64(eps))
    return p, m, v, norm
