"""Reference and error bound of the weight-EMA update, shared by test_ema_cpu.py and test_ema_gpu.py.

The update is ``e' = e + w (p - e)`` with ``w = float32(1 - decay_n)``; the reference evaluates it in
float64 from the fp32 inputs and the fp32 weight.

Bound.  An fp32 implementation computes ``fl(e + fl(w * fl(p - e)))``: three roundings, each with a
relative error ``|d_i| <= u = 2^-24`` (round to nearest):

    fl(p - e)      = (p - e)(1 + d1)
    fl(w * ...)    = w (p - e)(1 + d1)(1 + d2)              (+ at most 2^-150 when the product is subnormal)
    fl(e + ...)    = [e + w (p - e)(1 + d1)(1 + d2)](1 + d3)
                   = exact (1 + d3) + w (p - e)(d1 + d2 + d1 d2)(1 + d3)

so ``|result - exact| <= u |exact| + u (2 + u)(1 + u) w |p - e| + 2^-150 (1 + u)``, which is below

    ema_bound = 1.01 * 2^-24 * (2 w |p - e| + |exact|) + 2^-149.

The 1 % covers the second-order terms (~2^-23 relative) and the float64 evaluation of ``exact`` itself
(2^-53 relative).  A fused multiply-add drops d2, and the other association torch's lerp takes for
w >= 0.5, ``p - (p - e)(1 - w)``, has the same three roundings with ``(1 - w)|p - e| <= w |p - e|``
there (and ``1 - w`` exact in fp32 for w in [0.5, 1]); both stay inside the same bound.  Measured on
the CPU (test_ema_cpu.py): torch._foreach_lerp_, the update of get_ema_multi_avg_fn, reaches at most
0.990 of the bound over 2^20 log-spread Gaussian elements at decays 0.5 ... 0.9999, and is exact on
multiples of 1/8 at decays 0.5, 0.75, 0.875.
"""
import numpy as np
import torch


def decay_at(n, decay, warmup=False):
    """Decay of the update after ``n`` earlier ones: ``decay``, under warmup min(decay, (1+n)/(10+n))."""
    return min(decay, (1 + n) / (10 + n)) if warmup else decay


def weight32(n, decay, warmup=False):
    """The fp32 weight of update ``n`` (0-based): 1 for the first, else float32(1 - decay_n)."""
    return np.float32(1.0) if n == 0 else np.float32(1.0 - decay_at(n, decay, warmup))


def ema_step(e, p, w32):
    """float64 ``e + w (p - e)`` from fp32 tensors and the fp32 weight; w == 1 is a copy."""
    w32 = np.float32(w32)
    if w32 == np.float32(1.0):
        return p.double().clone()
    e, p = e.double(), p.double()
    return e + float(w32) * (p - e)


def ema_bound(e, p, w32):
    w = float(np.float32(w32))
    return 1.01 * 2.0 ** -24 * (2.0 * w * (p.double() - e.double()).abs() + ema_step(e, p, w32).abs()) + 2.0 ** -149


def eighths(n, gen, device="cpu"):
    """Multiples of 1/8 in [-8, 8]."""
    return (torch.randint(-64, 65, (n,), generator=gen, device=device).float() / 8.0)


def log_gaussians(n, gen, device="cpu"):
    """Gaussians with magnitudes spread over 1e-3 .. 1e3."""
    mag = 10.0 ** (6.0 * torch.rand(n, generator=gen, device=device) - 3.0)
    return (torch.randn(n, generator=gen, device=device) * mag).float()
