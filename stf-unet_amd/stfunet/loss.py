"""Training criterion on the gfx950 loss kernels.

Mirrors ``criterion`` (train_utils/train_and_eval.py:299-313): for every output
head, cross-entropy + multiclass Dice loss on the softmax
(train_utils/dice_coefficient_loss.py:5-55), ``losses['out'] + 0.5 *
losses['aux']`` when an aux head is present.  The reference's per-image Python
loop and its ``if sets_sum == 0`` host sync (dice_coefficient_loss.py:24-35)
become two kernels with a branch-free empty-set rule; the scalar loss stays on
the device.

The reference's three options run on the device as well:

* ``loss_weight``: per-class weights of the cross-entropy (torch's weighted mean:
  ``sum w[t] nll / sum w[t]``); they do not enter the Dice term.
* ``ignore_index >= 0``: pixels whose target equals it are left out of the cross-entropy
  and of every Dice sum, and get a gradient of exactly 0.  ``DriveDataset.collate_fn`` pads
  the targets of a mixed-size batch with 255, so such a batch trains with
  ``ignore_index=255``.  An image whose pixels are all ignored has Dice 1 (the reference's
  empty-set rule); a batch whose pixels are all ignored has a NaN loss, as
  ``F.cross_entropy`` gives -- not special-cased.
* ``dice=False``: cross-entropy only.

Two additions for lesion-sized foregrounds, after the reference's parameters:

* ``focal_gamma > 0``: each pixel's cross-entropy term is multiplied by ``(1 - p_t) ** focal_gamma``
  (``sum w[t] (1-p_t)^gamma nll / sum w[t]``: the denominator is unchanged), which down-weights the
  mass of easy pixels.  0 is the plain cross-entropy.
* ``tversky=(alpha, beta)``: the Tversky index ``(2I + eps) / (2I + 2 alpha FP + 2 beta FN + eps)``
  in place of Dice, with ``FP = sum p - I`` and ``FN = sum t - I`` per (image, class); ``beta > alpha``
  penalises missed foreground more than false alarms.  ``(0.5, 0.5)`` is Dice.  Needs ``dice=True``.

The four routes, resolved in one place (``_route``), first match first; more than 16 classes is a
ValueError:

1. a focal exponent or a Tversky pair: ``stf_loss_ft_fwd`` / ``stf_loss_ft_bwd``, 1 to 16 classes, every
   option included (anything but ``focal_gamma == 0`` and ``tversky is None``, ``(0.5, 0.5)`` too);
2. 5 to 16 classes: ``stf_loss_mc_fwd`` / ``stf_loss_mc_bwd``, the same formula with the options as
   run-time arguments (1. and 2. are one kernel family);
3. up to 4 classes in the reference's default configuration (no class weights, no ignored target value,
   Dice on): ``stf_loss_fwd`` / ``stf_loss_bwd``, which take no option arguments;
4. up to 4 classes otherwise: ``stf_loss_opt_fwd`` / ``stf_loss_opt_bwd`` (one kernel family with 3.).
"""
import math

import torch

from . import _lib
from .nhwc import _p, check_num_classes
from ._lib import call, stream


def _route(K, weight, ignore_index, dice, focal):
    """The entry points of one criterion call (module docstring, routes 1 to 4) and the option arguments
    they take between ``classes`` and ``terms``: (scratch, fwd, bwd, opts).  ``focal`` is (gamma, alpha,
    beta) or None."""
    opts = (_p(weight) if weight is not None else None, ignore_index, int(dice))
    if focal is not None:
        infix, opts = "ft_", opts + tuple(focal)
    elif K > 4:
        infix = "mc_"
    elif weight is None and dice and ignore_index < 0:
        infix, opts = "", ()
    else:
        infix = "opt_"
    return f"stf_loss_{infix}scratch_floats", f"stf_loss_{infix}fwd", f"stf_loss_{infix}bwd", opts


class _CEDice(torch.autograd.Function):
    """CE + Dice (+ focal / Tversky: ``focal`` = (gamma, alpha, beta), else None) through the entry points
    ``_route`` resolves."""

    @staticmethod
    def forward(ctx, logits, target, weight, ignore_index, dice, focal=None):
        logits = logits.detach().contiguous().float()
        target = target.contiguous()
        if target.dtype != torch.int64:
            target = target.long()
        N, K, H, W = logits.shape
        assert target.shape == (N, H, W), f"target {tuple(target.shape)} vs logits {tuple(logits.shape)}"
        scratch, fwd, ctx.bwd, ctx.opts = _route(K, weight, ignore_index, dice, focal)
        ctx.weight = weight                     # keeps the pointer in ctx.opts alive
        terms = torch.empty(getattr(_lib.load(), scratch)(N, K), dtype=torch.float32, device=logits.device)
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        call(fwd, _p(logits), _p(target), N, H, W, K, *ctx.opts, _p(terms), _p(loss), stream())
        ctx.save_for_backward(logits, target, terms)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        logits, target, terms = ctx.saved_tensors
        N, K, H, W = logits.shape
        go = grad_out.detach().float().contiguous().reshape(1)
        dl = torch.empty_like(logits)
        call(ctx.bwd, _p(logits), _p(target), N, H, W, K, *ctx.opts, _p(terms), _p(go), _p(dl), stream())
        return dl, None, None, None, None, None


def _class_weight(weight, num_classes, device=None):
    """``weight`` (tensor or sequence of ``num_classes`` floats) as a contiguous fp32 vector,
    on ``device`` when given; ValueError for another length."""
    if weight is None:
        return None
    w = torch.as_tensor(weight, dtype=torch.float32).detach().reshape(-1)
    if w.numel() != num_classes:
        raise ValueError(f"loss_weight has {w.numel()} entries for {num_classes} classes")
    if device is not None:
        w = w.to(device)
    return w.contiguous()


def _check_ignore(ignore_index, num_classes):
    if 0 <= ignore_index < num_classes:
        raise ValueError(f"ignore_index={ignore_index} is a class id (num_classes={num_classes}): the reference's "
                         "result there is an accident of its one-hot encoding")


def _focal_tversky(focal_gamma, tversky, dice):
    """None for the defaults (``focal_gamma == 0`` and ``tversky is None``), else the three floats
    (gamma, alpha, beta) of the focal / Tversky entry points; ValueError for a value they refuse."""
    try:
        gamma = float(focal_gamma)
    except (TypeError, ValueError):
        raise ValueError(f"focal_gamma={focal_gamma!r} is not a number") from None
    if not (math.isfinite(gamma) and gamma >= 0):
        raise ValueError(f"focal_gamma={focal_gamma!r} must be finite and >= 0")
    if tversky is None:
        return None if gamma == 0 else (gamma, 0.5, 0.5)
    try:
        alpha, beta = (float(v) for v in tversky)
    except (TypeError, ValueError):
        raise ValueError(f"tversky={tversky!r} must be None or a pair (alpha, beta)") from None
    if not (math.isfinite(alpha) and math.isfinite(beta) and alpha >= 0 and beta >= 0):
        raise ValueError(f"tversky={tversky!r}: alpha and beta must be finite and >= 0")
    if alpha == 0 and beta == 0:
        raise ValueError("tversky=(0, 0): alpha and beta must not both be 0")
    if not dice:
        raise ValueError("tversky replaces the Dice term: it needs dice=True")
    return gamma, alpha, beta


def ce_dice_loss(logits, target, weight=None, ignore_index=-100, dice=True, focal_gamma=0.0, tversky=None):
    ignore_index = int(ignore_index)
    K = logits.shape[1]
    check_num_classes(K)
    _check_ignore(ignore_index, K)
    focal = _focal_tversky(focal_gamma, tversky, dice)
    weight = _class_weight(weight, K, logits.device)
    if not logits.is_cuda:
        raise RuntimeError("stfunet loss kernels need a ROCm device (no CPU fallback)")
    return _CEDice.apply(logits, target, weight, ignore_index, bool(dice), focal)


def criterion(inputs, target, loss_weight=None, num_classes: int = 2, dice: bool = True, ignore_index: int = -100,
              focal_gamma: float = 0.0, tversky=None):
    """Same signature and reduction as the reference ``criterion``, then ``focal_gamma`` and ``tversky``.

    The defaults (the configuration the reference trains with, train_and_eval.py:395) take the
    fused default kernels; ``loss_weight`` (a tensor or a sequence of ``num_classes`` floats),
    ``ignore_index >= 0`` and ``dice=False`` take the option kernels (module docstring).
    ValueError for ``0 <= ignore_index < num_classes`` and for a weight vector whose length
    is not ``num_classes``.  A weight that is not yet a tensor on the logits' device is copied
    there on every call; a training loop converts it once (``engine.train_one_epoch`` does).

    ``focal_gamma`` (>= 0) and ``tversky`` (None or a pair ``(alpha, beta)``, >= 0 and not both 0,
    with ``dice=True``) are additions (module docstring); the same values go to every head.  Anything
    but ``focal_gamma=0, tversky=None`` takes the focal / Tversky kernels.  ValueError for a value
    outside those ranges.
    """
    check_num_classes(num_classes)
    _check_ignore(int(ignore_index), num_classes)
    _focal_tversky(focal_gamma, tversky, dice)
    loss_weight = _class_weight(loss_weight, num_classes)
    losses = {name: ce_dice_loss(x, target, loss_weight, ignore_index, dice, focal_gamma, tversky)
              for name, x in inputs.items()}
    if len(losses) == 1:
        return losses["out"]
    return losses["out"] + 0.5 * losses["aux"]
