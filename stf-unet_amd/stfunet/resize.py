"""Full-resolution logits: the bilinear resize kernels (``csrc/resize.hip``).

``STFLSTMUNet`` returns logits at H/2 x W/2, as the reference module does,
while ``DriveDataset`` yields full-resolution masks.  ``STFLSTMUNet(..., output_size="input")``
appends ``resize_fwd`` as the last op of its program (and ``resize_bwd`` as the first of its
backward); ``upsample_logits`` is the same pair as a stand-alone differentiable function.

The values are ``F.interpolate(logits, size=size, mode="bilinear", align_corners=False)``'s (the
same fp32 coordinate arithmetic).  Unlike torch's device backward, the gradient is a gather with a
fixed summation order: no atomics, bit-identical from run to run, and a library launch, so a
recorded plan (plan.py) contains it.
"""
import torch

from ._lib import call, stream
from .nhwc import _p, empty


def _check_size(h, w, size):
    H, W = (int(s) for s in size)
    if H < h or W < w:
        raise ValueError(f"upsample_logits only enlarges: target size {(H, W)} is smaller than the logits' {(h, w)}")
    return H, W


def resize_fwd(x, size):
    """``x`` [N, K, h, w] fp32 contiguous on the device -> a new [N, K, H, W] (a program buffer)."""
    N, K, h, w = x.shape
    H, W = size
    y = empty((N, K, H, W), torch.float32, x.device)
    call("stf_resize_bilinear_fwd", _p(x), N * K, h, w, _p(y), H, W, stream())
    return y


def resize_bwd(dy, size):
    """``dy`` [N, K, H, W] fp32 contiguous -> the gradient at ``size`` = (h, w), a new program buffer."""
    N, K, H, W = dy.shape
    h, w = size
    dx = empty((N, K, h, w), torch.float32, dy.device)
    call("stf_resize_bilinear_bwd", _p(dy), N * K, H, W, _p(dx), h, w, stream())
    return dx


class _Upsample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, size):
        x = logits.detach().contiguous()
        ctx.low = tuple(x.shape[-2:])
        return resize_fwd(x, size)

    @staticmethod
    def backward(ctx, dy):
        return resize_bwd(dy.detach().float().contiguous(), ctx.low), None


def upsample_logits(logits, size):
    """Bilinear resize (align_corners=False) of fp32 NCHW ``logits`` on the device up to
    ``size`` = (H, W), differentiable.  RuntimeError for a host tensor (no CPU fallback),
    ValueError for a target size smaller than the logits'."""
    if not logits.is_cuda:
        raise RuntimeError("stfunet resize kernels need a ROCm device (no CPU fallback)")
    if logits.dim() != 4 or logits.dtype != torch.float32:
        raise ValueError(f"upsample_logits expects fp32 [N, K, h, w] logits, got {logits.dtype} "
                         f"{tuple(logits.shape)}")
    size = _check_size(logits.shape[2], logits.shape[3], size)
    return _Upsample.apply(logits, size)
