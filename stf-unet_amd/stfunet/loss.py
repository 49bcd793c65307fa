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

The boundary term (``boundary_criterion(..., boundary_weight > 0)``; Kervadec et al., MIDL 2019) is added
behind whichever route runs: ``boundary_weight * L_B`` with ``L_B = sum m p_k phi_k / ((K-1) M)`` over the foreground classes
``k >= 1``, ``phi_k`` the signed distance map of ``target == k`` (``signed_distance_maps``), ``m`` the
``ignore_index`` mask and ``M = sum m``.  ``stf_bloss_fwd`` adds it to the route's loss on the same stream and
``stf_bloss_bwd`` adds its gradient into the route's ``dlogits``: one autograd node, no second gradient
tensor.  With ``boundary_weight == 0`` (the default) no boundary kernel runs and no map is made.

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
from ._lib import MAX_SIDE, call, stream


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
    def forward(ctx, logits, target, weight, ignore_index, dice, focal=None, boundary=None):
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
        ctx.boundary = None
        if boundary is not None:                # (weight, maps): the term is added to the route's loss
            alpha, phi = boundary
            ctx.boundary = (int(ignore_index), float(alpha))
            part = _bloss_fwd(logits, target, phi, *ctx.boundary, loss)
            ctx.save_for_backward(logits, target, terms, phi, part)
            return loss
        ctx.save_for_backward(logits, target, terms)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        logits, target, terms = ctx.saved_tensors[:3]
        N, K, H, W = logits.shape
        go = grad_out.detach().float().contiguous().reshape(1)
        dl = torch.empty_like(logits)
        call(ctx.bwd, _p(logits), _p(target), N, H, W, K, *ctx.opts, _p(terms), _p(go), _p(dl), stream())
        if ctx.boundary is not None:            # ... and its gradient into the route's dlogits
            phi, part = ctx.saved_tensors[3:]
            _bloss_bwd(logits, target, phi, *ctx.boundary, go, part, dl)
        return dl, None, None, None, None, None, None


def _bloss_fwd(logits, target, phi, ignore_index, alpha, loss):
    """``loss += alpha * L_B``; returns the partials (element 1 is M, which the backward reads)."""
    N, K, H, W = logits.shape
    part = torch.empty(_lib.load().stf_bloss_scratch_floats(N), dtype=torch.float32, device=logits.device)
    call("stf_bloss_fwd", _p(logits), _p(target), _p(phi), N, H, W, K, ignore_index, alpha, _p(part), _p(loss),
         stream())
    return part


def _bloss_bwd(logits, target, phi, ignore_index, alpha, go, part, dl):
    """``dl += go * alpha * dL_B/dlogits``"""
    N, K, H, W = logits.shape
    call("stf_bloss_bwd", _p(logits), _p(target), _p(phi), N, H, W, K, ignore_index, alpha, _p(go), _p(part[1:]),
         _p(dl), stream())


class _Boundary(torch.autograd.Function):
    """The bare term ``L_B``: the same two entry points on a zeroed loss and a zeroed gradient."""

    @staticmethod
    def forward(ctx, logits, target, phi, ignore_index):
        logits = logits.detach().contiguous().float()
        loss = torch.zeros((), dtype=torch.float32, device=logits.device)
        ctx.ignore_index = ignore_index
        part = _bloss_fwd(logits, target, phi, ignore_index, 1.0, loss)
        ctx.save_for_backward(logits, target, phi, part)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        logits, target, phi, part = ctx.saved_tensors
        go = grad_out.detach().float().contiguous().reshape(1)
        dl = torch.zeros_like(logits)
        _bloss_bwd(logits, target, phi, ctx.ignore_index, 1.0, go, part, dl)
        return dl, None, None, None


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


MAX_MAP = 1 << 31                # signed_distance_maps: H, W <= MAX_SIDE and N * (K-1) * H * W below this


def _boundary_weight(boundary_weight, num_classes):
    """``boundary_weight`` as a float; ValueError unless it is finite and >= 0, and for a positive weight
    with a single class (there is no foreground class)."""
    try:
        w = float(boundary_weight)
    except (TypeError, ValueError):
        raise ValueError(f"boundary_weight={boundary_weight!r} is not a number") from None
    if not (math.isfinite(w) and w >= 0):
        raise ValueError(f"boundary_weight={boundary_weight!r} must be finite and >= 0")
    if w > 0 and num_classes == 1:
        raise ValueError("boundary_weight > 0 needs a foreground class: num_classes must be at least 2")
    return w


def _no_ignore(ignore_index):
    """The map's and the term's ignore value as an int: None or a negative value is 'none' (-100)."""
    return -100 if ignore_index is None or int(ignore_index) < 0 else int(ignore_index)


def signed_distance_maps(target, num_classes, ignore_index=None):
    """float32 ``[N, K-1, H, W]`` on the target's device: the signed Euclidean distance maps of the boundary
    loss (Kervadec's ``one_hot2dist`` at unit spacing), one per foreground class ``k = 1..K-1`` in channel
    ``k-1`` (class 0 gets no map).  ``target`` is an integer ``[N, H, W]`` device tensor,
    ``2 <= num_classes <= 16``, ``H, W <= 4096``.  Per image and class, with ``G = {target == k}``:

    * outside ``G``: ``+d(q, G)``, the distance to the nearest pixel of ``G`` (at least 1);
    * inside ``G``: ``-(d(q, not G) - 1)``, so the innermost border of ``G`` gets 0;
    * ``G`` empty in that image: 0 everywhere (Kervadec's rule);
    * ``G`` the whole image: 0 everywhere as well (this project's rule; Kervadec's code does not
      special-case it and scipy's transform of an all-nonzero array returns an artefact);
    * pixels whose target equals ``ignore_index`` are in no ``G``: they count as "not G" (the 255 padding
      of ``collate_fn`` is not lesion) and still receive a value; the loss leaves them out, not the map.

    Exact: the squared distance is an integer and the value is ``float32(sqrt(float64(d2)))``, the bits of
    ``np.float32(scipy.ndimage.distance_transform_edt(...))``; the same bits from run to run and for an
    image alone or inside a batch.  The cost follows the pixel count, not the position of the sites.  The
    maps take ``N (K-1) H W * 4`` bytes (16.8 MB for 64 x 256 x 256 at K = 2)."""
    K = int(num_classes)
    if not 2 <= K <= 16:
        raise ValueError(f"num_classes={num_classes}: signed_distance_maps takes 2 to 16 classes")
    if target.dim() != 3:
        raise ValueError(f"target must be [N, H, W], not {tuple(target.shape)}")
    if target.dtype.is_floating_point or target.dtype.is_complex or target.dtype == torch.bool:
        raise ValueError(f"target must be an integer tensor, not {target.dtype}")
    N, H, W = target.shape
    if N and not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"target: H and W must be in 1..{MAX_SIDE}, not {H} x {W}")
    if N * (K - 1) * H * W >= MAX_MAP:
        raise ValueError(f"N * (K-1) * H * W must be below 2^31, not {N * (K - 1) * H * W}")
    ignore = _no_ignore(ignore_index)
    if not target.is_cuda:
        raise RuntimeError("signed_distance_maps needs a ROCm device (no CPU fallback)")
    phi = torch.empty((N, K - 1, H, W), dtype=torch.float32, device=target.device)
    if N:
        target = target.detach().to(torch.int64).contiguous()
        scratch = _lib.scratch_words(_lib.load().stf_sdf_scratch_bytes(N, H, W, K), target.device)
        with torch.cuda.device(target.device):
            call("stf_sdf", _p(target), N, H, W, K, ignore, _p(phi), _p(scratch), stream())
    return phi


def _check_dist(dist, logits):
    """A precomputed map for these logits: float32 ``[N, K-1, H, W]`` on their device, contiguous."""
    N, K, H, W = logits.shape
    if not torch.is_tensor(dist) or dist.dtype != torch.float32 or tuple(dist.shape) != (N, K - 1, H, W):
        got = (tuple(dist.shape), dist.dtype) if torch.is_tensor(dist) else type(dist).__name__
        raise ValueError(f"dist must be a float32 tensor of shape {(N, K - 1, H, W)}, not {got}")
    if dist.device != logits.device:
        raise ValueError(f"dist is on {dist.device}, the logits on {logits.device}")
    return dist.detach().contiguous()


def _int64(target):
    target = target.contiguous()
    return target if target.dtype == torch.int64 else target.long()


def boundary_loss(logits, target, ignore_index=-100, dist=None):
    """The bare boundary term ``L_B = sum m p_k phi_k / ((K-1) M)`` (module docstring) as a differentiable
    device scalar, for users who blend it themselves.  ``dist``: precomputed ``signed_distance_maps`` of
    this target (made here when None).  The value is in pixels, of the order of the mean distance to the
    contour, so useful weights are small (0.01 and rising).  NaN when every pixel is ignored."""
    ignore_index = int(ignore_index)
    if logits.dim() != 4:
        raise ValueError(f"logits must be [N, K, H, W], not {tuple(logits.shape)}")
    K = logits.shape[1]
    check_num_classes(K)
    if K == 1:
        raise ValueError("boundary_loss needs a foreground class: at least 2 classes")
    _check_ignore(ignore_index, K)
    if dist is not None:
        dist = _check_dist(dist, logits)
    if not logits.is_cuda:
        raise RuntimeError("stfunet loss kernels need a ROCm device (no CPU fallback)")
    if dist is None:
        dist = signed_distance_maps(target, K, ignore_index)
    return _Boundary.apply(logits, _int64(target), dist, _no_ignore(ignore_index))


def ce_dice_loss(logits, target, weight=None, ignore_index=-100, dice=True, focal_gamma=0.0, tversky=None):
    return ce_dice_boundary_loss(logits, target, weight, ignore_index, dice, focal_gamma, tversky)


def ce_dice_boundary_loss(logits, target, weight=None, ignore_index=-100, dice=True, focal_gamma=0.0, tversky=None,
                          boundary_weight=0.0, dist=None):
    """``ce_dice_loss`` of one head plus ``boundary_weight`` times the boundary term, in one autograd node;
    ``dist``: precomputed ``signed_distance_maps`` of this target (made here when None).  With
    ``boundary_weight == 0`` it is ``ce_dice_loss``: no map, no boundary kernel, the same bits."""
    ignore_index = int(ignore_index)
    K = logits.shape[1]
    check_num_classes(K)
    _check_ignore(ignore_index, K)
    focal = _focal_tversky(focal_gamma, tversky, dice)
    weight = _class_weight(weight, K, logits.device)
    boundary_weight = _boundary_weight(boundary_weight, K)
    if boundary_weight > 0 and dist is not None:
        dist = _check_dist(dist, logits)
    if not logits.is_cuda:
        raise RuntimeError("stfunet loss kernels need a ROCm device (no CPU fallback)")
    if boundary_weight == 0:
        return _CEDice.apply(logits, target, weight, ignore_index, bool(dice), focal)
    if dist is None:
        dist = signed_distance_maps(target, K, ignore_index)
    return _CEDice.apply(logits, target, weight, ignore_index, bool(dice), focal, (boundary_weight, dist))


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


def boundary_criterion(inputs, target, loss_weight=None, num_classes: int = 2, dice: bool = True,
                       ignore_index: int = -100, focal_gamma: float = 0.0, tversky=None,
                       boundary_weight: float = 0.0):
    """``criterion`` with its parameters, then ``boundary_weight`` (finite, >= 0): that many times the boundary
    term ``L_B`` (module docstring, ``signed_distance_maps``) is added to every head's loss.  ``criterion`` keeps
    the reference's parameter list; the option lives here.

    The maps are made once per call from ``target`` and shared by the heads (``out + 0.5 * aux`` as in
    ``criterion``).  ``L_B`` is in pixels, so useful weights are small (0.01, raised from epoch to epoch).
    With ``boundary_weight == 0`` this is ``criterion`` itself: no map, no boundary kernel, the same bits.
    ValueError for a negative or non-finite weight and for a positive one with ``num_classes == 1``, before
    any device work, beside ``criterion``'s own.
    """
    check_num_classes(num_classes)
    _check_ignore(int(ignore_index), num_classes)
    _focal_tversky(focal_gamma, tversky, dice)
    boundary_weight = _boundary_weight(boundary_weight, num_classes)
    if boundary_weight == 0:
        return criterion(inputs, target, loss_weight, num_classes, dice, ignore_index, focal_gamma, tversky)
    loss_weight = _class_weight(loss_weight, num_classes)
    if not all(x.is_cuda for x in inputs.values()):
        raise RuntimeError("stfunet loss kernels need a ROCm device (no CPU fallback)")
    dist = signed_distance_maps(target, num_classes, int(ignore_index))
    losses = {name: ce_dice_boundary_loss(x, target, loss_weight, ignore_index, dice, focal_gamma, tversky,
                                          boundary_weight, dist)
              for name, x in inputs.items()}
    if len(losses) == 1:
        return losses["out"]
    return losses["out"] + 0.5 * losses["aux"]
