"""Inference on the device: masks, per-image Dice / IoU and overlays.

The reference's inference script (``test.py:146-176``) with its helpers restated on the
gfx950 kernels of ``csrc/predict.hip``:

* ``predict_masks``   logits -> ``uint8`` mask (``torch.sigmoid(outputs) > 0.5``, test.py:168-169,
  or the argmax ``evaluate`` scores) and, with a target, the per-image (|P&T|, |P|, |T|) counts
* ``image_metrics``   counts -> per-image Dice and IoU (``compute_metrics``,
  train_utils/visualize.py:9-50), on the device, no host synchronisation
* ``boundary_metrics``  per-image Hausdorff distance, HD95 and ASSD of mask against target
  (MedPy's ``hd`` / ``hd95`` / ``assd`` at isotropic spacing; ``csrc/boundary.hip``), and
  ``distance_transform_sq``, the exact squared Euclidean distance transform underneath
* ``connected_components`` / ``filter_components``  per-image component labels in
  ``scipy.ndimage.label``'s numbering, and the usual clean-up of a predicted mask (keep the largest
  component, drop components below a size) with the counts of the cleaned mask (``csrc/ccl.hip``)
* ``overlay``         the mask painted over a frame (``save_overlay_from_tensor``, test.py:52-82,
  through ``merge_images``, train_utils/merge_tumor_images.py:94-120)
* ``predict``         the loop: eval mode, ``no_grad``, ``preprocess_input``, forward, masks,
  counts when the loader yields targets, one PNG per slice when ``output_dir`` is given
* ``flip_planes`` / ``tta_probabilities`` / ``predict_tta``  mirror test-time augmentation: the model
  on the batch and its flipped copies, the un-flipped class probabilities averaged in a fixed order
  (``csrc/tta.hip``), and ``predict``'s loop with each batch's mask taken from that mean
* ``connected_components_3d`` / ``filter_components_3d`` / ``predict_volumes``  the same labels and
  clean-up per volume of stacked slices (6 / 18 / 26 connectivity, the same ``csrc/ccl.hip``), and the loop
  that groups a patient's slices: 3-D post-processing and per-volume (per-case) Dice / IoU
* ``boundary_metrics_3d`` / ``distance_transform_3d``  per-volume HD, HD95 and ASSD with voxel spacing
  ``(sz, sy, sx)`` (MedPy on the 3-D array) and the weighted squared distance transform underneath
  (the volume kernels of ``csrc/boundary.hip``); ``predict_volumes(boundary=True)`` reports them per case

* ``lesion_metrics`` / ``lesion_metrics_3d``  lesion-level detection per image / per volume: target lesions
  found and missed, predicted components that are false findings, and the (area, hit) table of either
  side (the lesion kernels of ``csrc/ccl.hip``); ``predict_volumes(lesions=True)`` and
  ``predict_tta(lesions=True)`` report lesion-level sensitivity, precision and false findings

``predict(model, loader, device, rule="sigmoid", channel=0, paint=0)`` reproduces test.py bit for
bit (it thresholds channel 0 and inverts the mask before painting, :75-76), except that the
PNGs are RGB: channel ``c`` of an overlay takes ``color[c]``, where the reference hands the same
triple to cv2 as B, G, R.  The default colour (0, 255, 0) reads the same both ways.

* ``score_histogram`` / ``threshold_curves``  threshold-free evaluation: the per-image histogram of the
  foreground score split by the target (``csrc/curves.hip``) and, from it, every operating point
  (Dice / IoU per threshold and the best one), AUROC, average precision and the calibration table with
  its ECE; ``predict_tta(curves=True)`` and ``predict_volumes(curves=True)`` report them per image / case

* ``lesion_scores`` / ``lesion_scores_3d`` / ``froc_curves``  the lesion metrics swept over the confidence of
  each predicted component: per candidate the largest score row of its voxels, per target lesion the
  largest confidence among the matched candidates that touch it, the three-sided histogram of both
  (the FROC passes of ``csrc/ccl.hip``) and, from it, lesion sensitivity against false findings per case
  at every confidence; ``predict_tta(froc=True)`` and ``predict_volumes(froc=True)`` report them

There is no CPU path: tensors on the host raise (``threshold_curves`` and ``froc_curves`` are torch ops and
take a table on any device).
"""
import numbers
import os

import torch

from ._lib import MAX_SIDE, call, load, scratch_words, stream
from .nhwc import _p

RULES = {"argmax": 0, "sigmoid": 1, "threshold": 2}
VIEWS = {"none": 0, "w": 1, "h": 2, "hw": 3}        # flip code: bit 0 = the last axis W, bit 1 = H
ALL_VIEWS = ("none", "w", "h", "hw")
MAX_CLASSES = 16
MAX_PIXELS = 1 << 31             # boundary metrics / distance transform: H, W <= MAX_SIDE and B * H * W below this
MAX_FULL_SCAN = 1 << 32          # distance_transform_sq without `where`: B * H * W * H at most this


def _device_only(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"stfunet.predict.{what} runs the gfx950 predict kernels: tensors must be on a ROCm "
                           "device (no CPU fallback)")


def _check_target_shape(target, shape):
    if tuple(target.shape) != tuple(shape):
        raise ValueError(f"target {tuple(target.shape)} does not match the mask's {tuple(shape)}")


def _check_target_dtype(target):
    if target.dtype.is_floating_point or target.dtype.is_complex or target.dtype == torch.bool:
        raise ValueError(f"target must be an integer tensor, not {target.dtype}")


def _check_target(target, shape):
    """``target`` must be an integer tensor of the mask's ``shape``."""
    _check_target_shape(target, shape)
    _check_target_dtype(target)


def _ignore(ignore_index):
    """The entry points' ``ignore_index``: -1 for none."""
    return -1 if ignore_index is None else ignore_index


def _check_paint(color, alpha, paint):
    color = tuple(color)
    if len(color) != 3 or any(int(c) != c or not 0 <= c <= 255 for c in color):
        raise ValueError(f"color must be three integers in 0..255, not {color}")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha must be in [0, 1], not {alpha}")
    if paint not in (0, 1):
        raise ValueError(f"paint must be 0 (colour where the mask is zero) or 1, not {paint}")
    return tuple(int(c) for c in color)


def predict_masks(outputs, rule="argmax", channel=0, threshold=0.5, target=None, ignore_index=None):
    """``uint8 [B, H, W]`` mask of logits ``[B, K, H, W]`` (or the models' ``{"out": logits}``).

    ``rule="argmax"``: the class id of the first maximum (``torch.argmax(outputs, 1)``).
    ``rule="sigmoid"``: ``torch.sigmoid(outputs[:, channel]) > threshold`` in fp32.
    ``rule="threshold"``: ``outputs[:, channel] > threshold`` with no sigmoid, for planes that hold
    probabilities already (``tta_probabilities``); a NaN compares false.
    With ``target`` (``[B, H, W]`` integers) also returns ``int64 [B, 3]`` per-image counts
    (|P&T|, |P|, |T|) with P = mask > 0 and T = target > 0; pixels whose target equals
    ``ignore_index`` are left out of all three."""
    if isinstance(outputs, dict):
        outputs = outputs["out"]
    if rule not in RULES:
        raise ValueError(f"unknown rule {rule!r} (one of {sorted(RULES)})")
    if outputs.dim() != 4:
        raise ValueError(f"logits must be [B, K, H, W], not {tuple(outputs.shape)}")
    B, K, H, W = outputs.shape
    if not 1 <= K <= MAX_CLASSES:
        raise ValueError(f"1..{MAX_CLASSES} classes are supported, not {K}")
    if not 0 <= channel < K:
        raise ValueError(f"channel {channel} is outside [0, {K})")
    if target is not None and tuple(target.shape) != (B, H, W):
        raise ValueError(f"target {tuple(target.shape)} does not match the logits' {(B, H, W)}")
    _device_only(outputs, "predict_masks")
    x = outputs.detach().float().contiguous()
    mask = torch.empty((B, H, W), dtype=torch.uint8, device=x.device)
    counts = None
    if target is not None:
        target = target.detach().to(device=x.device, dtype=torch.int64).contiguous()
        counts = torch.empty((B, 3), dtype=torch.int64, device=x.device)
    with torch.cuda.device(x.device):
        if rule == "threshold":
            call("stf_predict_threshold", _p(x), _p(target), B, K, H * W, channel, threshold, _ignore(ignore_index),
                 _p(mask), _p(counts), stream())
        else:
            call("stf_predict_mask", _p(x), _p(target), B, K, H * W, RULES[rule], channel, threshold,
                 _ignore(ignore_index), _p(mask), _p(counts), stream())
    return mask if target is None else (mask, counts)


def image_metrics(counts, smooth=1e-5):
    """Per-image ``dice = (2I + s) / (P + T + s)`` and ``iou = (I + s) / (P + T - I + s)`` of
    ``[B, 3]`` counts (I, P, T), as float64 tensors on the counts' device."""
    c = counts.to(torch.float64)
    inter, p, t = c.unbind(-1)
    return (2 * inter + smooth) / (p + t + smooth), (inter + smooth) / (p + t - inter + smooth)


def _as_u8(t, what):
    """``t`` as a contiguous uint8 tensor, nonzero where ``t`` is (bool and uint8 are not copied)."""
    if t.dtype.is_floating_point or t.dtype.is_complex:
        raise ValueError(f"{what} must be bool or an integer tensor, not {t.dtype}")
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    elif t.dtype != torch.uint8:
        t = (t != 0).view(torch.uint8)
    return t.contiguous()


def _check_bhw(t, what):
    if t.dim() != 3:
        raise ValueError(f"{what} must be [B, H, W], not {tuple(t.shape)}")
    B, H, W = t.shape
    if B and not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"{what}: H and W must be in 1..{MAX_SIDE}, not {H} x {W}")
    if B * H * W >= MAX_PIXELS:
        raise ValueError(f"{what}: B * H * W must be below 2^31, not {B * H * W}")
    return B, H, W


def _check_spacing(spacing):
    if isinstance(spacing, bool) or not isinstance(spacing, numbers.Real) or not 0.0 < spacing < float("inf"):
        raise ValueError(f"spacing must be a finite positive number, not {spacing!r}")
    return float(spacing)


def _boundary_scratch(B, H, W, device):
    """The scratch of the image boundary entry points"""
    return scratch_words(load().stf_boundary_scratch_bytes(B, H, W), device)


def _checked_sites(sites, where, name):
    """The transforms' checked ``sites`` and ``where`` (None stays None) of one shape: contiguous uint8 on
    the sites' device."""
    if where is not None and tuple(where.shape) != tuple(sites.shape):
        raise ValueError(f"where {tuple(where.shape)} does not match the sites' {tuple(sites.shape)}")
    sites = _as_u8(sites.detach(), "sites")
    _device_only(sites, name)
    if where is not None:
        where = _as_u8(where.detach(), "where")
        _device_only(where, name)
        where = where.to(sites.device)
    return sites, where


def boundary_metrics(mask, target, ignore_index=None, spacing=1.0):
    """Per-image boundary metrics of ``mask`` against ``target`` (both ``[B, H, W]``; ``mask`` bool,
    uint8 or any integer, nonzero = foreground; ``target`` any integer, > 0 = foreground; pixels
    whose target equals ``ignore_index`` are background on both sides).

    Returns ``{"hd", "hd95", "assd"}`` as float64 ``[B]`` device tensors and ``border_counts``
    int64 ``[B, 2]`` = (|dP|, |dT|).  The border of M is ``M & ~erode(M)`` with the 4-neighbour
    cross and background outside the image; distances are Euclidean between border pixels in both
    directions, times ``spacing``: HD their maximum, HD95 numpy's linear 95th percentile of all of
    them, ASSD half the sum of the two directions' means (MedPy's hd / hd95 / assd).  An image
    with an empty mask or target gets NaN in all three."""
    _check_target_shape(target, mask.shape)
    B, H, W = _check_bhw(mask, "mask")
    spacing = _check_spacing(spacing)
    _check_target_dtype(target)
    mask = _as_u8(mask.detach(), "mask")
    _device_only(mask, "boundary_metrics")
    _device_only(target, "boundary_metrics")
    dev = mask.device
    out = torch.empty((B, 3), dtype=torch.float64, device=dev)
    counts = torch.empty((B, 2), dtype=torch.int64, device=dev)
    if B:
        target = target.detach().to(device=dev, dtype=torch.int64).contiguous()
        scratch = _boundary_scratch(B, H, W, dev)
        with torch.cuda.device(dev):
            call("stf_boundary_metrics", _p(mask), _p(target), B, H, W, _ignore(ignore_index), _p(out), _p(counts),
                 _p(scratch), stream())
        if spacing != 1.0:
            out = out * spacing
    hd, hd95, assd = out.unbind(1)
    return {"hd": hd, "hd95": hd95, "assd": assd, "border_counts": counts}


def distance_transform_sq(sites, where=None):
    """int32 ``[B, H, W]``: the exact squared Euclidean distance of every pixel to the nearest
    nonzero pixel of ``sites`` (bool or integer ``[B, H, W]``); ``INT32_MAX`` everywhere in an image
    without sites.  With ``where`` (same shape) only its nonzero pixels are computed, the others
    are -1.

    The column pass scans outward from each computed pixel, so a pixel costs about the distance it
    finds, at worst H row reads.  Without ``where`` every pixel is computed, and sparse sites in a
    large image make that one long kernel; such a call is refused (``ValueError``) when its bound
    ``B * H * W * H`` exceeds ``MAX_FULL_SCAN`` (2^32: a batch of 64 at 256 x 256 is 2^30, one
    1024 x 1024 image 2^30, one 2048 x 2048 image 2^33).  Passing ``where`` (all ones, if every pixel
    is wanted) lifts the guard: the caller then owns the cost."""
    B, H, W = _check_bhw(sites, "sites")
    if where is None and B * H * W * H > MAX_FULL_SCAN:
        raise ValueError(f"distance_transform_sq without `where` may read B * H * W * H = {B * H * W * H} rows "
                         f"(more than {MAX_FULL_SCAN}) when the sites are sparse; pass `where` to name the pixels "
                         "that are needed, or all ones to accept the cost")
    sites, where = _checked_sites(sites, where, "distance_transform_sq")
    d2 = torch.empty((B, H, W), dtype=torch.int32, device=sites.device)
    if B:
        scratch = _boundary_scratch(B, H, W, sites.device)
        with torch.cuda.device(sites.device):
            call("stf_edt_sq", _p(sites), _p(where), B, H, W, _p(d2), _p(scratch), stream())
    return d2


CONNECTIVITIES = (4, 8)


def _check_components(connectivity, min_size=0):
    if isinstance(connectivity, bool) or connectivity not in CONNECTIVITIES:
        raise ValueError(f"connectivity must be 4 (edge neighbours) or 8 (edges and corners), not {connectivity!r}")
    if isinstance(min_size, bool) or not isinstance(min_size, numbers.Integral) or not 0 <= min_size < 1 << 63:
        raise ValueError(f"min_size must be an integer >= 0, not {min_size!r}")
    return int(connectivity), int(min_size)


CONNECTIVITIES_3D = (6, 18, 26)


def _check_components_3d(connectivity, min_size=0):
    if isinstance(connectivity, bool) or connectivity not in CONNECTIVITIES_3D:
        raise ValueError(f"connectivity must be 6 (faces), 18 (faces and edges) or 26 (faces, edges and corners), "
                         f"not {connectivity!r}")
    _, min_size = _check_components(8, min_size)
    return int(connectivity), min_size


def _check_depths(depths, total=None):
    """``depths`` as a list of ints: positive integers (no bools) that sum to ``total`` when that is
    given; ``None`` is one volume of ``total`` slices."""
    if depths is None:
        depths = [total] if total else []
    elif isinstance(depths, (str, bytes, numbers.Number)):
        raise ValueError(f"depths must be a sequence of positive integers, not {depths!r}")
    else:
        try:
            depths = list(depths)
        except TypeError:
            raise ValueError(f"depths must be a sequence of positive integers, not {depths!r}") from None
    for d in depths:
        if isinstance(d, bool) or not isinstance(d, numbers.Integral) or d < 1:
            raise ValueError(f"depths must be positive integers, not {d!r}")
    depths = [int(d) for d in depths]
    if total is not None and sum(depths) != total:
        raise ValueError(f"depths sum to {sum(depths)}, but there are {total} slices")
    return depths


def _starts(depths, device):
    """The volume table of the 3-D entry points: (host int32 [V + 1], its device copy)."""
    host = torch.zeros(len(depths) + 1, dtype=torch.int32)
    host[1:] = torch.tensor(depths, dtype=torch.int64).cumsum(0)
    return host, host.to(device)


def _ccl_call(op, mask, depths, before, after):
    """One component entry point on a checked uint8 device mask, with its scratch: ``stf_ccl_<op>``
    per image (``depths`` None) or ``stf_ccl3d_<op>`` per volume of checked ``depths``.  ``before`` are
    the arguments ahead of ``N, H, W``, ``after`` those from ``connectivity`` up to the scratch."""
    N, H, W = mask.shape
    dev = mask.device
    with torch.cuda.device(dev):
        if depths is None:
            scratch = scratch_words(load().stf_ccl_scratch_bytes(N, H, W), dev)
            call("stf_ccl_" + op, *before, N, H, W, *after, _p(scratch), stream())
        else:
            V = len(depths)
            host, starts = _starts(depths, dev)               # the call reads the host table before it returns
            scratch = scratch_words(load().stf_ccl3d_scratch_bytes(N, H, W, V), dev)
            call("stf_ccl3d_" + op, *before, N, H, W, _p(starts), host.data_ptr(), V, *after, _p(scratch), stream())


def _label(mask, depths, connectivity):
    """``stf_ccl_label`` / ``stf_ccl3d_label`` on a checked uint8 device mask: (labels, num int32 [B or V])."""
    N, H, W = mask.shape
    labels = torch.empty((N, H, W), dtype=torch.int32, device=mask.device)
    num = torch.empty((N if depths is None else len(depths),), dtype=torch.int32, device=mask.device)
    if N:
        _ccl_call("label", mask, depths, (_p(mask),), (connectivity, _p(labels), _p(num)))
    return labels, num


def _filter(mask, target, depths, keep_largest, min_size, connectivity, ignore_index):
    """``stf_ccl_filter`` / ``stf_ccl3d_filter`` on a checked uint8 device mask: (filtered mask, counts
    or None, num), counts and num per image (``depths`` None) or per volume."""
    N, H, W = mask.shape
    dev = mask.device
    V = N if depths is None else len(depths)
    out = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    num = torch.empty((V,), dtype=torch.int32, device=dev)
    counts = None
    if target is not None:
        target = target.detach().to(device=dev, dtype=torch.int64).contiguous()
        counts = torch.empty((V, 3), dtype=torch.int64, device=dev)
    if N:
        _ccl_call("filter", mask, depths, (_p(mask), _p(target)),
                  (connectivity, int(bool(keep_largest)), min_size, _ignore(ignore_index), _p(out), _p(counts), _p(num)))
    return out, counts, num


def _checked_mask(mask, target, what):
    """The uint8 device mask of a component call; ``target`` (or None) must match it and be on the device."""
    if target is not None:
        _check_target(target, mask.shape)
    mask = _as_u8(mask.detach(), "mask")
    _device_only(mask, what)
    if target is not None:
        _device_only(target, what)
    return mask


def connected_components(mask, connectivity=8):
    """``(labels int32 [B, H, W], num int32 [B])``: the connected components of every image of
    ``mask`` (``[B, H, W]`` bool or any integer, nonzero = foreground), each image on its own.

    ``connectivity`` 4 joins edge neighbours, 8 edges and corners; pixels outside the image are
    background.  ``labels`` is 0 on the background and 1..n on the components, numbered per image in
    raster order of each component's first pixel -- ``scipy.ndimage.label(mask[b],
    generate_binary_structure(2, 1 or 2))`` -- and ``num[b]`` is n.  Integers only: the same bits
    from run to run."""
    _check_bhw(mask, "mask")
    connectivity, _ = _check_components(connectivity)
    return _label(_checked_mask(mask, None, "connected_components"), None, connectivity)


def filter_components(mask, keep_largest=False, min_size=0, connectivity=8, target=None, ignore_index=None):
    """``uint8 [B, H, W]``: ``mask`` (``[B, H, W]`` bool or any integer, nonzero = foreground) with the
    components that do not pass set to 0, each image on its own.

    A component (``connected_components``) passes when its area is at least ``min_size`` pixels and,
    with ``keep_largest``, it is the largest of its image; of several largest ones the one whose first
    pixel comes first in raster order is kept (``np.argmax(np.bincount(labels.ravel())[1:])``).
    ``min_size`` applies first: an image whose largest component is smaller comes out empty.  A pixel
    that stays keeps its own value, so a mask of class ids keeps them (integer masks wider than
    uint8 are reduced to 0 / 1 first).  With ``target`` (``[B, H, W]`` integers) returns ``(mask,
    counts)``, ``counts`` the ``int64 [B, 3]`` (|P&T|, |P|, |T|) of the filtered mask with
    ``predict_masks``' rules (``ignore_index`` pixels left out of all three, but labelled like any
    other pixel).  With neither option set the output equals the input; the call still runs the
    kernels."""
    _check_bhw(mask, "mask")
    connectivity, min_size = _check_components(connectivity, min_size)
    mask = _checked_mask(mask, target, "filter_components")
    out, counts, _ = _filter(mask, target, None, keep_largest, min_size, connectivity, ignore_index)
    return out if target is None else (out, counts)


def connected_components_3d(mask, depths=None, connectivity=26):
    """``(labels int32 [N, H, W], num int32 [V])``: the connected components of the volumes of
    ``mask`` (``[N, H, W]`` bool or any integer, nonzero = foreground), a stack of slices cut into
    ``V = len(depths)`` volumes of ``depths[v]`` consecutive slices (``None``: one volume), each
    volume on its own -- volumes never touch, whatever their adjacent slices hold.

    ``connectivity`` 6 joins face neighbours, 18 faces and edges, 26 faces, edges and corners; voxels
    outside the volume are background.  ``labels`` is 0 on the background and 1..n on the components,
    numbered per volume in raster order (z, y, x) of each component's first voxel --
    ``scipy.ndimage.label(volume, generate_binary_structure(3, 1, 2 or 3))`` -- and ``num[v]`` is n.
    Integers only: the same bits from run to run."""
    N, H, W = _check_bhw(mask, "mask")
    connectivity, _ = _check_components_3d(connectivity)
    depths = _check_depths(depths, N)
    return _label(_checked_mask(mask, None, "connected_components_3d"), depths, connectivity)


def filter_components_3d(mask, depths=None, keep_largest=False, min_size=0, connectivity=26, target=None,
                         ignore_index=None):
    """``uint8 [N, H, W]``: ``filter_components`` per volume instead of per image.  ``mask`` is a stack
    of slices cut into volumes by ``depths`` as in ``connected_components_3d``.

    A component passes when it has at least ``min_size`` voxels and, with ``keep_largest``, it is the
    largest of its volume; of several largest ones the one whose first voxel comes first in raster
    order (z, y, x) is kept.  ``min_size`` applies first.  A voxel that stays keeps its own value.
    With ``target`` (``[N, H, W]`` integers) returns ``(mask, counts)``, ``counts`` the ``int64 [V, 3]``
    (|P&T|, |P|, |T|) of the filtered mask summed over each volume with ``predict_masks``' rules;
    ``image_metrics(counts)`` is then the per-volume Dice / IoU."""
    N, H, W = _check_bhw(mask, "mask")
    connectivity, min_size = _check_components_3d(connectivity, min_size)
    depths = _check_depths(depths, N)
    mask = _checked_mask(mask, target, "filter_components_3d")
    out, counts, _ = _filter(mask, target, depths, keep_largest, min_size, connectivity, ignore_index)
    return out if target is None else (out, counts)


def _is_real(x):
    return isinstance(x, numbers.Real) and not isinstance(x, bool)


MAX_LESIONS = 1 << 20            # rows of a lesion table: a limit on the argument, not on the counts


def _check_lesions(min_overlap, max_lesions=0):
    if not _is_real(min_overlap) or not 0.0 <= min_overlap <= 1.0:
        raise ValueError(f"min_overlap must be a number in [0, 1], not {min_overlap!r}")
    if isinstance(max_lesions, bool) or not isinstance(max_lesions, numbers.Integral) or \
            not 0 <= max_lesions <= MAX_LESIONS:
        raise ValueError(f"max_lesions must be an integer in 0..{MAX_LESIONS}, not {max_lesions!r}")
    return float(min_overlap), int(max_lesions)


def _lesions(mask, target, depths, connectivity, min_overlap, max_lesions, ignore_index):
    """``stf_lesion_metrics`` / ``stf_lesion3d_metrics`` on a checked uint8 device mask: (summary int64
    [V, 4], table int64 [V, 2, max_lesions, 2] or None), per image (``depths`` None) or per volume."""
    N, H, W = mask.shape
    dev = mask.device
    V = N if depths is None else len(depths)
    summary = torch.empty((V, 4), dtype=torch.int64, device=dev)
    table = torch.empty((V, 2, max_lesions, 2), dtype=torch.int64, device=dev) if max_lesions else None
    if N:
        target = target.detach().to(device=dev, dtype=torch.int64).contiguous()
        after = (connectivity, min_overlap, max_lesions, _ignore(ignore_index), _p(summary), _p(table))
        with torch.cuda.device(dev):
            scratch = scratch_words(load().stf_lesion_scratch_bytes(N, H, W, V), dev)
            if depths is None:
                call("stf_lesion_metrics", _p(mask), _p(target), N, H, W, *after, _p(scratch), stream())
            else:
                host, starts = _starts(depths, dev)           # the call reads the host table before it returns
                call("stf_lesion3d_metrics", _p(mask), _p(target), N, H, W, _p(starts), host.data_ptr(), V, *after,
                     _p(scratch), stream())
    return summary, table


def _lesion_result(summary, table):
    """The dict of ``lesion_metrics``: the summary's columns and the two ratios, torch ops on the device."""
    n_t, m_t, n_p, m_p = summary.unbind(1)
    res = {"n_target": n_t, "matched_target": m_t, "n_pred": n_p, "matched_pred": m_p,
           "sensitivity": m_t.to(torch.float64) / n_t.to(torch.float64),        # 0 / 0 = NaN
           "precision": m_p.to(torch.float64) / n_p.to(torch.float64)}
    if table is not None:
        res["lesions"] = table
    return res


def lesion_metrics(mask, target, connectivity=8, min_overlap=0.0, max_lesions=64, ignore_index=None):
    """Lesion-level detection metrics of ``mask`` against ``target``, per image (both ``[B, H, W]``;
    ``mask`` bool, uint8 or any integer, nonzero = foreground; ``target`` any integer, > 0 = foreground;
    pixels whose target equals ``ignore_index`` are background on both sides before labelling).

    Either side is labelled on its own (``connected_components`` at ``connectivity``).  A target lesion
    has an ``area`` and a ``hit`` (its pixels under the predicted foreground), a predicted component
    likewise against the target foreground; either is matched iff ``hit >= 1`` and
    ``float(hit) >= min_overlap * float(area)`` (``min_overlap`` in [0, 1]; 0: any overlap).

    Returns a dict of device tensors: int64 ``[B]`` ``n_target``, ``matched_target`` (lesions found; the
    rest were missed), ``n_pred``, ``matched_pred`` (the rest are false findings), float64
    ``sensitivity = matched_target / n_target`` and ``precision = matched_pred / n_pred`` (NaN where the
    denominator is 0) and, unless ``max_lesions`` is 0, ``lesions`` int64 ``[B, 2, max_lesions, 2]``: side
    0 the target, side 1 the prediction, row ``l - 1`` = (area, hit) of label ``l``, zero past ``n``;
    labels above ``max_lesions`` are left out of the table but still counted.  Integers only: the same
    bits from run to run; no host synchronisation."""
    _check_target_shape(target, mask.shape)
    _check_bhw(mask, "mask")
    connectivity, _ = _check_components(connectivity)
    min_overlap, max_lesions = _check_lesions(min_overlap, max_lesions)
    mask = _checked_mask(mask, target, "lesion_metrics")
    return _lesion_result(*_lesions(mask, target, None, connectivity, min_overlap, max_lesions, ignore_index))


def lesion_metrics_3d(mask, target, depths=None, connectivity=26, min_overlap=0.0, max_lesions=64,
                      ignore_index=None):
    """``lesion_metrics`` per volume (per case) instead of per image: ``mask`` and ``target`` are stacks
    of slices ``[N, H, W]`` cut into ``V = len(depths)`` volumes as in ``connected_components_3d``
    (connectivity 6, 18 or 26); every tensor of the result has ``V`` rows.  The same bits for a volume
    passed alone or inside a stack."""
    _check_target_shape(target, mask.shape)
    N, H, W = _check_bhw(mask, "mask")
    connectivity, _ = _check_components_3d(connectivity)
    depths = _check_depths(depths, N)
    min_overlap, max_lesions = _check_lesions(min_overlap, max_lesions)
    mask = _checked_mask(mask, target, "lesion_metrics_3d")
    return _lesion_result(*_lesions(mask, target, depths, connectivity, min_overlap, max_lesions, ignore_index))


def _pooled_lesions(summaries, per):
    """The lesion keys of the predict loops from the per-flush summaries (None without targets)."""
    keys = ("lesion_counts", "lesion_sensitivity", "lesion_precision", "false_findings", "false_findings_per_" + per)
    if not summaries:
        return dict.fromkeys(keys)
    counts = torch.cat(summaries)
    tot = counts.sum(0).to(torch.float64)
    false = counts[:, 2] - counts[:, 3]
    return dict(zip(keys, (counts, tot[1] / tot[0], tot[3] / tot[2], false, false.to(torch.float64).mean())))


def _check_spacing_3d(spacing, V):
    """``spacing`` of the volume calls as ``V`` rows ``[sz, sy, sx]`` of floats: a positive finite
    number (isotropic), one triple ``(sz, sy, sx)`` for every volume, or ``V`` triples (a sequence or
    a ``[V, 3]`` tensor; a tensor on the device is copied to the host to be checked)."""
    what = (f"spacing must be a finite positive number, a triple (sz, sy, sx) of such numbers or one triple per "
            f"volume ({V}), not {spacing!r}")
    if torch.is_tensor(spacing):
        if spacing.dim() not in (1, 2) or spacing.dtype in (torch.bool,) or spacing.dtype.is_complex:
            raise ValueError(what)
        spacing = spacing.detach().to("cpu", torch.float64).tolist()
    if _is_real(spacing):
        rows = [[spacing] * 3] * V
    elif isinstance(spacing, (str, bytes)) or spacing is None:
        raise ValueError(what)
    else:
        try:
            items = list(spacing)
        except TypeError:
            raise ValueError(what) from None
        if len(items) == 3 and all(_is_real(s) for s in items):
            rows = [items] * V
        else:
            rows = []
            for item in items:
                if isinstance(item, (str, bytes)) or _is_real(item) or isinstance(item, bool) or item is None:
                    raise ValueError(what)
                try:
                    row = item.tolist() if torch.is_tensor(item) else list(item)
                except TypeError:
                    raise ValueError(what) from None
                if len(row) != 3 or not all(_is_real(s) for s in row):
                    raise ValueError(what)
                rows.append(row)
            if len(rows) != V:
                raise ValueError(what)
    rows = [[float(s) for s in row] for row in rows]
    if not all(0.0 < s < float("inf") for row in rows for s in row):
        raise ValueError(what)
    return rows


def _boundary3d(mask, target, depths, rows, ignore_index):
    """``stf_boundary3d_metrics`` on a checked uint8 device mask with checked ``depths`` and spacing
    ``rows``: (out float64 [V, 3], border counts int64 [V, 2])."""
    N, H, W = mask.shape
    dev, V = mask.device, len(depths)
    out = torch.empty((V, 3), dtype=torch.float64, device=dev)
    counts = torch.empty((V, 2), dtype=torch.int64, device=dev)
    if N:
        target = target.detach().to(device=dev, dtype=torch.int64).contiguous()
        host, starts = _starts(depths, dev)                   # the call reads the host table before it returns
        spacing = torch.tensor(rows, dtype=torch.float64).reshape(V, 3).to(dev)
        scratch = scratch_words(load().stf_boundary3d_scratch_bytes(N, H, W, V), dev)
        with torch.cuda.device(dev):
            call("stf_boundary3d_metrics", _p(mask), _p(target), N, H, W, _p(starts), host.data_ptr(), V, _p(spacing),
                 _ignore(ignore_index), _p(out), _p(counts), _p(scratch), stream())
    return out, counts


def boundary_metrics_3d(mask, target, depths=None, spacing=1.0, ignore_index=None):
    """Per-volume (per-case) boundary metrics of ``mask`` against ``target`` (both ``[N, H, W]``, a
    stack of slices cut into ``V = len(depths)`` volumes as in ``connected_components_3d``; ``mask``
    bool, uint8 or any integer, nonzero = foreground; ``target`` any integer, > 0 = foreground; voxels
    whose target equals ``ignore_index`` are background on both sides).

    Returns ``{"hd", "hd95", "assd"}`` as float64 ``[V]`` device tensors in the unit of ``spacing`` and
    ``border_counts`` int64 ``[V, 2]`` = (|dP|, |dT|): MedPy's ``hd`` / ``hd95`` / ``assd`` on each
    volume with ``voxelspacing=(sz, sy, sx)`` and ``connectivity=1``.  The border of M is
    ``M & ~erode(M)`` with the 6-neighbour cross and background outside the volume (so in a volume
    one slice deep every foreground voxel is a border voxel, unlike ``boundary_metrics``); volumes
    never see each other.  ``spacing``: a positive finite number, a triple ``(sz, sy, sx)`` or one
    triple per volume (a sequence or a ``[V, 3]`` tensor).  A volume with an empty mask or target
    gets NaN in all three.  The same bits from run to run, and for a volume passed alone or in a
    stack."""
    _check_target_shape(target, mask.shape)
    N, H, W = _check_bhw(mask, "mask")
    depths = _check_depths(depths, N)
    rows = _check_spacing_3d(spacing, len(depths))
    _check_target_dtype(target)
    mask = _as_u8(mask.detach(), "mask")
    _device_only(mask, "boundary_metrics_3d")
    _device_only(target, "boundary_metrics_3d")
    out, counts = _boundary3d(mask, target, depths, rows, ignore_index)
    hd, hd95, assd = out.unbind(1)
    return {"hd": hd, "hd95": hd95, "assd": assd, "border_counts": counts}


def distance_transform_3d(sites, depths=None, spacing=1.0, where=None):
    """float64 ``[N, H, W]``: the squared distance, weighted by ``spacing``, of every voxel to the
    nearest nonzero voxel of ``sites`` (bool or integer ``[N, H, W]``) of the same volume (``depths``
    and ``spacing`` as in ``boundary_metrics_3d``); ``+inf`` throughout a volume without sites.  With
    ``where`` (same shape) only its nonzero voxels are computed, the others are -1.

    The plane pass scans along ``y`` in every slice that has a site and the depth pass along ``z``
    from every computed voxel, each about as far as the distance found.  Without ``where`` a call
    whose bound ``N * H * W * (H + max(depths))`` exceeds ``MAX_FULL_SCAN`` is refused
    (``ValueError``); passing ``where`` (all ones, if every voxel is wanted) lifts the guard."""
    N, H, W = _check_bhw(sites, "sites")
    depths = _check_depths(depths, N)
    rows = _check_spacing_3d(spacing, len(depths))
    bound = N * H * W * (H + max(depths, default=0))
    if where is None and bound > MAX_FULL_SCAN:
        raise ValueError(f"distance_transform_3d without `where` may read N * H * W * (H + depth) = {bound} values "
                         f"(more than {MAX_FULL_SCAN}) when the sites are sparse; pass `where` to name the voxels "
                         "that are needed, or all ones to accept the cost")
    sites, where = _checked_sites(sites, where, "distance_transform_3d")
    dev, V = sites.device, len(depths)
    d2 = torch.empty((N, H, W), dtype=torch.float64, device=dev)
    if N:
        host, starts = _starts(depths, dev)
        table = torch.tensor(rows, dtype=torch.float64).reshape(V, 3).to(dev)
        scratch = scratch_words(load().stf_boundary3d_scratch_bytes(N, H, W, V), dev)
        with torch.cuda.device(dev):
            call("stf_edt3d_sq", _p(sites), _p(where), N, H, W, _p(starts), host.data_ptr(), V, _p(table), _p(d2),
                 _p(scratch), stream())
    return d2


SOURCES = {"softmax": 0, "sigmoid": 1, "probs": 2}
MAX_BINS = 4096


def _is_int(x):
    return isinstance(x, numbers.Integral) and not isinstance(x, bool)


def _check_bins(bins):
    if not _is_int(bins) or not 2 <= bins <= MAX_BINS or bins & (bins - 1):
        raise ValueError(f"bins must be a power of two in [2, {MAX_BINS}], not {bins!r}")
    return int(bins)


def _check_hist_options(positive, ignore_index):
    if positive is not None and (not _is_int(positive) or positive < 0):
        raise ValueError(f"positive must be None (target > 0) or a class id >= 0, not {positive!r}")
    if ignore_index is not None and not _is_int(ignore_index):
        raise ValueError(f"ignore_index must be None or an integer, not {ignore_index!r}")


def _score_hist(scores, target, source, channel, bins, positive, ignore_index):
    """One ``stf_score_hist`` launch on checked device tensors: int64 ``[N, 2, bins + 1]``."""
    N, K, H, W = scores.shape
    hist = torch.empty((N, 2, bins + 1), dtype=torch.int64, device=scores.device)
    if N:
        target = target.detach().to(device=scores.device, dtype=torch.int64).contiguous()
        with torch.cuda.device(scores.device):
            call("stf_score_hist", _p(scores), N, K, H, W, SOURCES[source], channel, _p(target),
                 -1 if positive is None else positive, _ignore(ignore_index), bins, _p(hist), stream())
    return hist


def score_histogram(scores, target, source="probs", channel=0, bins=256, positive=None, ignore_index=None,
                    depths=None):
    """int64 ``[N, 2, bins + 1]``: per image, the histogram of the foreground score split by the target --
    the one object every threshold-free figure (``threshold_curves``) is made of.

    ``scores`` is fp32 ``[N, K, H, W]`` (or ``[N, H, W]``, one plane) on the device; the score ``p`` of a
    pixel is, by ``source``: ``"probs"`` plane ``channel`` as it is, ``"sigmoid"`` ``torch.sigmoid`` of
    logit plane ``channel`` (``predict_masks``' arithmetic), ``"softmax"`` plane ``channel`` of the
    softmax over the ``K`` logit planes (``tta_probabilities``' arithmetic, bit for bit).  With ``bins``
    a power of two in [2, 4096]::

        row(p) = 0                                        if not (p > 0)    # 0, -0, negatives, NaN
               = min(bins, int(ceil(float32(p * bins))))  otherwise         # +inf and p > 1: row bins

    so row ``j >= 1`` holds ``(j - 1) / bins < p <= j / bins`` and the rows above ``j`` are exactly the
    pixels ``predict_masks(rule="threshold", threshold=j / bins)`` marks.  ``hist[n, 1]`` counts the
    pixels with ``target > 0`` (``positive=None``) or ``target == positive``, ``hist[n, 0]`` all others;
    pixels whose target equals ``ignore_index`` are in neither.  ``depths`` (as in
    ``connected_components_3d``) sums the rows of each volume's slices on the device: ``[V, 2, bins + 1]``,
    the same bits for a volume passed alone or in a stack.  Integers only: the same bits from run to
    run; one launch, no host synchronisation."""
    if isinstance(scores, dict):
        scores = scores["out"]
    if source not in SOURCES:
        raise ValueError(f"unknown source {source!r} (one of {sorted(SOURCES)})")
    if scores.dim() == 3:
        scores = scores.unsqueeze(1)
    if scores.dim() != 4:
        raise ValueError(f"scores must be [N, K, H, W] or [N, H, W], not {tuple(scores.shape)}")
    if not scores.dtype.is_floating_point:
        raise ValueError(f"scores must be a floating-point tensor, not {scores.dtype}")
    N, K, H, W = scores.shape
    if not 1 <= K <= MAX_CLASSES:
        raise ValueError(f"1..{MAX_CLASSES} planes are supported, not {K}")
    if not _is_int(channel) or not 0 <= channel < K:
        raise ValueError(f"channel {channel!r} is outside [0, {K})")
    bins = _check_bins(bins)
    _check_hist_options(positive, ignore_index)
    _check_target(target, (N, H, W))
    _check_bhw(target, "target")
    if depths is not None:
        depths = _check_depths(depths, N)
    _device_only(scores, "score_histogram")
    _device_only(target, "score_histogram")
    hist = _score_hist(scores.detach().float().contiguous(), target, source, int(channel), bins, positive,
                       ignore_index)
    if depths is None:
        return hist
    volume = torch.repeat_interleave(torch.arange(len(depths)), torch.tensor(depths, dtype=torch.int64))
    return torch.zeros((len(depths), 2, bins + 1), dtype=torch.int64,
                       device=hist.device).index_add_(0, volume.to(hist.device), hist)


def _first_max(values):
    """(index, value) of the first maximum along the last axis -- the lowest index among equals."""
    best = values.max(-1, keepdim=True).values
    index = torch.arange(values.shape[-1], device=values.device)
    first = torch.where(values == best, index, values.shape[-1] - 1).min(-1).values
    return first, best.squeeze(-1)


def threshold_curves(hist, cal_groups=16, smooth=1e-5):
    """Every operating point, the ranking figures and the calibration of a score histogram ``hist``
    (``[..., 2, bins + 1]`` integers from ``score_histogram``; leading axes are kept), as a dict of
    tensors on ``hist``'s device -- torch ops in int64 / float64, no host synchronisation.

    With ``TP_j`` / ``FP_j`` the positives / negatives in the rows above ``j``, ``j = 0..bins`` -- the
    counts ``predict_masks(rule="threshold", threshold=j / bins)`` gives:

    * ``thresholds`` ``[bins + 1]`` = ``j / bins``; ``tp``, ``fp``, ``fn``, ``tn`` int64 ``[..., bins + 1]``
    * ``dice``, ``iou``: ``image_metrics`` of ``(TP, TP + FP, TP + FN)`` at ``smooth``, so every point equals
      the loops' figure bit for bit; ``best_threshold`` / ``best_dice``: the first maximum of ``dice`` (the
      lowest threshold among equals)
    * ``auroc``: the trapezoid rule over the points ``(FPR_j, TPR_j)`` preceded by ``(1, 1)``;
      ``average_precision``: ``sum_k (R_k - R_{k+1}) Prec_k`` over the rows ``k`` in descending order with
      the rows ``>= k`` predicted and precision 1 where nothing is.  These are scikit-learn's
      ``roc_auc_score`` / ``average_precision_score`` of the quantised scores (the rows); both are NaN when
      a side is empty.
    * ``reliability`` ``[..., G, 3]`` = (count, mean confidence, positive fraction) of ``G = cal_groups``
      equal-width groups (``G`` divides ``bins``; group ``g`` holds rows ``g * bins / G + 1 .. (g + 1) * bins / G``,
      row 0 joins group 0), the confidence of row ``j >= 1`` being its midpoint ``(j - 0.5) / bins`` and of
      row 0 zero, and ``ece`` = ``sum_g count_g / total * |positive fraction_g - mean confidence_g|`` (empty
      groups add nothing; NaN without pixels).  Every score is within ``1 / (2 bins)`` of its row's
      midpoint, so ``ece`` is within ``1 / (2 bins)`` of the expected calibration error of the same groups
      on the unquantised scores."""
    if hist.dim() < 2 or hist.shape[-2] != 2 or hist.shape[-1] < 3:
        raise ValueError(f"hist must be [..., 2, bins + 1], not {tuple(hist.shape)}")
    if hist.dtype.is_floating_point or hist.dtype.is_complex or hist.dtype == torch.bool:
        raise ValueError(f"hist must be an integer tensor, not {hist.dtype}")
    bins = _check_bins(hist.shape[-1] - 1)
    if not _is_int(cal_groups) or cal_groups < 1 or bins % cal_groups:
        raise ValueError(f"cal_groups must be a positive integer that divides bins = {bins}, not {cal_groups!r}")
    G = int(cal_groups)
    hist = hist.to(torch.int64)
    total = hist.sum(-1, keepdim=True)                        # [..., 2, 1]
    above = total - hist.cumsum(-1)                           # rows > j
    fp, tp = above.unbind(-2)
    n_neg, n_pos = total.unbind(-2)
    fn, tn = n_pos - tp, n_neg - fp
    dice, iou = image_metrics(torch.stack((tp, tp + fp, tp + fn), -1), smooth)
    f64 = torch.float64
    thresholds = torch.arange(bins + 1, dtype=f64, device=hist.device) / bins
    best, best_dice = _first_max(dice)
    # ranking: 0 / 0 = NaN marks an empty side
    tpr, fpr = tp.to(f64) / n_pos.to(f64), fp.to(f64) / n_neg.to(f64)
    one = torch.ones_like(tpr[..., :1])
    x, y = torch.cat((one, fpr), -1), torch.cat((one, tpr), -1)
    auroc = ((x[..., :-1] - x[..., 1:]) * (y[..., :-1] + y[..., 1:])).sum(-1) * 0.5
    at = torch.flip(hist, (-1,)).cumsum(-1)                   # rows >= k, k = bins .. 0
    fp_k, tp_k = at.to(f64).unbind(-2)
    recall = tp_k / n_pos.to(f64)
    precision = torch.where(tp_k + fp_k > 0, tp_k / (tp_k + fp_k), 1.0)
    step = recall - torch.cat((torch.zeros_like(recall[..., :1]), recall[..., :-1]), -1)
    ap = (step * precision).sum(-1)
    empty = ((n_pos == 0) | (n_neg == 0)).squeeze(-1)
    nan = torch.full_like(ap, float("nan"))
    auroc, ap = torch.where(empty, nan, auroc), torch.where(empty, nan, ap)
    # calibration
    rows = hist.sum(-2).to(f64)                               # [..., bins + 1]
    confidence = (torch.arange(1, bins + 1, dtype=f64, device=hist.device) - 0.5) / bins
    lead = hist.shape[:-2]
    count = rows[..., 1:].reshape(*lead, G, bins // G).sum(-1)
    count = torch.cat((count[..., :1] + rows[..., :1], count[..., 1:]), -1)
    conf_sum = (rows[..., 1:] * confidence).reshape(*lead, G, bins // G).sum(-1)
    pos_sum = hist[..., 1, 1:].to(f64).reshape(*lead, G, bins // G).sum(-1)
    pos_sum = torch.cat((pos_sum[..., :1] + hist[..., 1, :1].to(f64), pos_sum[..., 1:]), -1)
    mean_conf, pos_frac = conf_sum / count, pos_sum / count
    gap = torch.where(count > 0, count * (pos_frac - mean_conf).abs(), 0.0)
    ece = gap.sum(-1) / count.sum(-1)
    return {"thresholds": thresholds, "tp": tp, "fp": fp, "fn": fn, "tn": tn, "dice": dice, "iou": iou,
            "best_threshold": thresholds[best], "best_dice": best_dice, "auroc": auroc, "average_precision": ap,
            "reliability": torch.stack((count, mean_conf, pos_frac), -1), "ece": ece}


CURVE_KEYS = ("score_hist", "curves", "case_auroc", "case_average_precision", "mean_case_dice_curve",
              "best_case_threshold")


def _check_curves(curves, curve_bins, curve_channel):
    """The loops' checked curve options: (on, bins, channel); the two are not looked at while it is off."""
    if not curves:
        return False, curve_bins, curve_channel
    if not _is_int(curve_channel) or curve_channel < 0:
        raise ValueError(f"curve_channel must be a class id >= 0, not {curve_channel!r}")
    return True, _check_bins(curve_bins), int(curve_channel)


def _batch_hist(outputs, targets, views, rule, channel, bins, curve_channel, ignore_index):
    """The loops' one ``stf_score_hist`` launch per batch on what ``_batches`` yields: logits by ``rule``
    (softmax of class ``curve_channel``, or the sigmoid of the rule's own plane ``channel``), mean
    probabilities and ``rule="threshold"`` planes as they are."""
    if isinstance(outputs, dict):
        outputs = outputs["out"]
    source, plane = _loop_score(views, rule, channel, curve_channel)
    return score_histogram(outputs, targets, source, plane, bins, None, ignore_index)


def _loop_score(views, rule, channel, curve_channel):
    """(source, plane) of the loops' score in what ``_batches`` yields: logits by ``rule`` (softmax of class
    ``curve_channel``, or the sigmoid of the rule's own plane ``channel``), mean probabilities and
    ``rule="threshold"`` planes as they are."""
    if rule == "argmax":
        return ("softmax" if views is None else "probs"), curve_channel
    if rule == "sigmoid":
        return ("sigmoid", channel) if views is None else ("probs", 0)
    return "probs", channel


def _curve_result(hist):
    """The curve keys of the predict loops from the per-image or per-case histograms (None without targets)."""
    if hist is None:
        return dict.fromkeys(CURVE_KEYS)
    groups = min(16, hist.shape[-1] - 1)                       # threshold_curves' 16, or curve_bins below that
    per_case = threshold_curves(hist, groups)
    pooled = threshold_curves(hist.sum(0), groups)
    mean_dice = per_case["dice"].mean(0)
    best, _ = _first_max(mean_dice)
    return dict(zip(CURVE_KEYS, (hist, pooled, per_case["auroc"], per_case["average_precision"], mean_dice,
                                 pooled["thresholds"][best])))


FROC_RATES = (0.125, 0.25, 0.5, 1, 2, 4, 8)        # false findings per case of the LUNA16 performance metric
FROC_KEYS = ("froc_hist", "froc", "lesion_scores")


def _checked_scores(scores, shape, source, channel, bins):
    """``scores`` of the FROC calls as ``[N, K, H, W]`` for a mask of ``shape`` with the checked ``channel``
    and ``bins``: ``score_histogram``'s checks and messages."""
    if isinstance(scores, dict):
        scores = scores["out"]
    if source not in SOURCES:
        raise ValueError(f"unknown source {source!r} (one of {sorted(SOURCES)})")
    if scores.dim() == 3:
        scores = scores.unsqueeze(1)
    if scores.dim() != 4:
        raise ValueError(f"scores must be [N, K, H, W] or [N, H, W], not {tuple(scores.shape)}")
    if not scores.dtype.is_floating_point:
        raise ValueError(f"scores must be a floating-point tensor, not {scores.dtype}")
    N, K, H, W = scores.shape
    if not 1 <= K <= MAX_CLASSES:
        raise ValueError(f"1..{MAX_CLASSES} planes are supported, not {K}")
    if not _is_int(channel) or not 0 <= channel < K:
        raise ValueError(f"channel {channel!r} is outside [0, {K})")
    bins = _check_bins(bins)
    if (N, H, W) != tuple(shape):
        raise ValueError(f"scores {(N, H, W)} do not match the mask's {tuple(shape)}")
    return scores, int(channel), bins


def _froc(mask, scores, target, depths, source, channel, bins, connectivity, min_overlap, max_lesions, ignore_index):
    """``stf_froc`` / ``stf_froc3d`` on a checked uint8 device mask and checked device scores: (summary int64
    [V, 4], table int64 [V, 2, max_lesions, 3] or None, hist int64 [V, 3, bins + 1]), per image (``depths``
    None) or per volume."""
    N, H, W = mask.shape
    K = scores.shape[1]
    dev = mask.device
    V = N if depths is None else len(depths)
    summary = torch.empty((V, 4), dtype=torch.int64, device=dev)
    table = torch.empty((V, 2, max_lesions, 3), dtype=torch.int64, device=dev) if max_lesions else None
    hist = torch.empty((V, 3, bins + 1), dtype=torch.int64, device=dev)
    if N:
        target = target.detach().to(device=dev, dtype=torch.int64).contiguous()
        scores = scores.detach().to(device=dev, dtype=torch.float32).contiguous()
        before = (_p(mask), _p(scores), K, SOURCES[source], channel, _p(target), N, H, W)
        after = (connectivity, min_overlap, max_lesions, _ignore(ignore_index), bins, _p(summary), _p(table), _p(hist))
        with torch.cuda.device(dev):
            scratch = scratch_words(load().stf_froc_scratch_bytes(N, H, W, V, bins), dev)
            if depths is None:
                call("stf_froc", *before, *after, _p(scratch), stream())
            else:
                host, starts = _starts(depths, dev)           # the call reads the host table before it returns
                call("stf_froc3d", *before, _p(starts), host.data_ptr(), V, *after, _p(scratch), stream())
    return summary, table, hist


def _froc_result(summary, table, hist):
    res = _lesion_result(summary, table)
    res["froc_hist"] = hist
    return res


def lesion_scores(mask, scores, target, source="probs", channel=0, bins=256, connectivity=8, min_overlap=0.0,
                  max_lesions=64, ignore_index=None):
    """``lesion_metrics`` with a confidence for every predicted component and a detection score for every
    target lesion, per image: what a FROC curve is made of (``froc_curves``).

    ``mask``, ``target``, ``connectivity``, ``min_overlap``, ``max_lesions`` and ``ignore_index`` are
    ``lesion_metrics``'; every component of the prediction side is a candidate.  ``scores`` (fp32
    ``[B, K, H, W]`` or ``[B, H, W]`` on the device), ``source``, ``channel`` and ``bins`` are
    ``score_histogram``'s: the score ``p`` of a pixel and its ``row(p)`` in ``0..bins``.  Then

    * ``conf(c)`` = the largest ``row(p)`` over the pixels of candidate ``c``;
    * a candidate is matched by ``lesion_metrics``' rule (``hit >= 1`` and ``float(hit) >= min_overlap *
      float(area)``); every other candidate is a false finding;
    * ``det(t)`` = the largest ``conf(c)`` over the matched candidates that share a pixel with lesion ``t``,
      0 without one: a candidate that fails ``min_overlap`` lends nothing to the lesions it grazes.

    Returns ``lesion_metrics``' dict (the same bits) with two differences: ``lesions`` is int64 ``[B, 2,
    max_lesions, 3]``, row ``l - 1`` = (area, hit, score) of label ``l`` with score = ``det`` on side 0 (the
    target) and ``conf`` on side 1 (the prediction); and ``froc_hist`` int64 ``[B, 3, bins + 1]`` is added:
    side 0 counts the false findings by ``conf``, side 1 the target lesions by ``det`` (row 0: the lesions
    no matched candidate reached), side 2 the matched candidates by ``conf``, so the sides sum to
    ``n_pred - matched_pred``, ``n_target`` and ``matched_pred``.  Integers only: the same bits from run to
    run; no host synchronisation."""
    scores, channel, bins = _checked_scores(scores, mask.shape, source, channel, bins)
    _check_target_shape(target, mask.shape)
    _check_bhw(mask, "mask")
    connectivity, _ = _check_components(connectivity)
    min_overlap, max_lesions = _check_lesions(min_overlap, max_lesions)
    mask = _checked_mask(mask, target, "lesion_scores")
    _device_only(scores, "lesion_scores")
    return _froc_result(*_froc(mask, scores, target, None, source, channel, bins, connectivity, min_overlap,
                               max_lesions, ignore_index))


def lesion_scores_3d(mask, scores, target, depths=None, source="probs", channel=0, bins=256, connectivity=26,
                     min_overlap=0.0, max_lesions=64, ignore_index=None):
    """``lesion_scores`` per volume (per case) instead of per image: ``mask``, ``scores`` and ``target`` are
    stacks of slices cut into ``V = len(depths)`` volumes as in ``lesion_metrics_3d`` (connectivity 6, 18 or
    26); every tensor of the result has ``V`` rows.  The same bits for a volume passed alone or inside a
    stack."""
    scores, channel, bins = _checked_scores(scores, mask.shape, source, channel, bins)
    _check_target_shape(target, mask.shape)
    N, H, W = _check_bhw(mask, "mask")
    connectivity, _ = _check_components_3d(connectivity)
    depths = _check_depths(depths, N)
    min_overlap, max_lesions = _check_lesions(min_overlap, max_lesions)
    mask = _checked_mask(mask, target, "lesion_scores_3d")
    _device_only(scores, "lesion_scores_3d")
    return _froc_result(*_froc(mask, scores, target, depths, source, channel, bins, connectivity, min_overlap,
                               max_lesions, ignore_index))


def froc_curves(hist, cases=None, rates=FROC_RATES):
    """The FROC curve of a confidence histogram ``hist`` (``froc_hist`` of ``lesion_scores``): ``[3, bins + 1]``
    integers of ``cases`` cases (default 1), or ``[V, 3, bins + 1]``, which is summed over its ``V`` rows first
    (``cases`` default ``V``).  A dict of tensors on ``hist``'s device, which may be the host -- torch ops in
    int64 / float64, no host synchronisation.

    With ``X_j`` the sum of a side's rows above ``j``, ``j = 0..bins`` -- the candidates and lesions whose
    confidence exceeds ``j / bins``; point ``j`` thresholds the confidences of a fixed candidate set, it does
    not label the mask again:

    * ``thresholds`` ``[bins + 1]`` = ``j / bins``; int64 ``detected`` = ``X_j`` of side 1, ``false_findings`` of
      side 0, ``matched`` of side 2, and ``n_lesions``, all rows of side 1
    * ``sensitivity`` = ``detected / n_lesions`` (NaN without lesions), ``fp_per_case`` = ``false_findings /
      cases``, ``precision`` = ``matched / (matched + false_findings)``, 1 where nothing is predicted
    * ``sensitivity_at`` ``[len(rates)]``: for a rate ``r`` of false findings per case, ``sensitivity[j*]`` at the
      smallest ``j`` with ``float(false_findings[j]) <= r * float(cases)`` (``j = bins`` always qualifies): a
      step function, nothing is interpolated; and ``cpm``, their mean -- at the default rates the LUNA16
      competition performance metric.  NaN without lesions."""
    if hist.dim() not in (2, 3) or hist.shape[-2] != 3 or hist.shape[-1] < 3:
        raise ValueError(f"hist must be [3, bins + 1] or [V, 3, bins + 1], not {tuple(hist.shape)}")
    if hist.dtype.is_floating_point or hist.dtype.is_complex or hist.dtype == torch.bool:
        raise ValueError(f"hist must be an integer tensor, not {hist.dtype}")
    bins = _check_bins(hist.shape[-1] - 1)
    pooled = hist.dim() == 3
    if cases is None:
        cases = hist.shape[0] if pooled else 1
    if not _is_real(cases) or not cases > 0:
        raise ValueError(f"cases must be a number > 0, not {cases!r}")
    try:
        rates = [r for r in rates]
    except TypeError:
        raise ValueError(f"rates must be a sequence of numbers >= 0, not {rates!r}") from None
    if not rates or not all(_is_real(r) and r >= 0 for r in rates):
        raise ValueError(f"rates must be a non-empty sequence of numbers >= 0, not {rates!r}")
    hist = hist.to(torch.int64)
    if pooled:
        hist = hist.sum(0)
    f64 = torch.float64
    total = hist.sum(-1, keepdim=True)                        # [3, 1]
    false, detected, matched = (total - hist.cumsum(-1)).unbind(0)   # rows > j
    n_lesions = total[1, 0]
    sensitivity = detected.to(f64) / n_lesions.to(f64)        # 0 / 0 = NaN
    predicted = (matched + false).to(f64)
    precision = torch.where(predicted > 0, matched.to(f64) / predicted, 1.0)
    limit = torch.tensor([float(r) for r in rates], dtype=f64, device=hist.device) * float(cases)
    index = torch.arange(bins + 1, device=hist.device)
    first = torch.where(false.to(f64)[None, :] <= limit[:, None], index, bins).min(-1).values
    sensitivity_at = sensitivity[first]
    return {"thresholds": index.to(f64) / bins, "detected": detected, "false_findings": false, "matched": matched,
            "n_lesions": n_lesions, "sensitivity": sensitivity, "fp_per_case": false.to(f64) / float(cases),
            "precision": precision, "sensitivity_at": sensitivity_at, "cpm": sensitivity_at.mean()}


def _check_froc(froc, froc_bins, froc_overlap, curve_channel):
    """The loops' checked FROC options: (on, bins, overlap); nothing is looked at while it is off."""
    if not froc:
        return False, froc_bins, froc_overlap
    if not _is_int(curve_channel) or curve_channel < 0:
        raise ValueError(f"curve_channel must be a class id >= 0, not {curve_channel!r}")
    return True, _check_bins(froc_bins), _check_lesions(froc_overlap)[0]


def _batch_froc(mask, outputs, targets, depths, views, rule, channel, curve_channel, bins, connectivity, overlap,
                ignore_index):
    """The loops' one ``stf_froc`` / ``stf_froc3d`` call per batch / flush: the reported mask against the score
    ``curves=True`` uses (``_loop_score``), the table at ``lesion_scores``' 64 rows."""
    source, plane = _loop_score(views, rule, channel, curve_channel)
    scores, plane, bins = _checked_scores(outputs, mask.shape, source, plane, bins)
    return _froc(mask, scores, targets, depths, source, plane, bins, connectivity, overlap, 64, ignore_index)


def _froc_loop_result(parts):
    """The FROC keys of the predict loops from the per-batch / per-flush (summary, table, hist) (None without
    targets): the tables per image / case and the curve of the pooled one, one case per row."""
    if not parts:
        return dict.fromkeys(FROC_KEYS)
    hist = torch.cat([p[2] for p in parts])
    return dict(zip(FROC_KEYS, (hist, froc_curves(hist), torch.cat([p[1] for p in parts]))))


def overlay(frames, mask, color=(0, 255, 0), alpha=0.5, paint=1):
    """``uint8 [B, H, W, 3]``: ``frames`` normalised to 0..255 per image, with ``color`` blended
    at ``alpha`` into the pixels where the mask is non-zero (``paint=1``) or zero (``paint=0``).

    ``frames`` is ``[B, H, W]`` fp32, contiguous or any view whose last two dimensions are
    (``inputs[:, 0, 0]`` of a ``[B, T, C, H, W]`` batch is read in place).  Frames with
    non-finite pixels give an undefined picture."""
    color = _check_paint(color, alpha, paint)
    if frames.dim() != 3:
        raise ValueError(f"frames must be [B, H, W], not {tuple(frames.shape)}")
    if tuple(mask.shape) != tuple(frames.shape):
        raise ValueError(f"mask {tuple(mask.shape)} does not match the frames' {tuple(frames.shape)}")
    _device_only(frames, "overlay")
    _device_only(mask, "overlay")
    B, H, W = frames.shape
    frames = frames.detach()
    if frames.dtype != torch.float32:
        frames = frames.float()
    if B and H * W and (frames.stride(2) != 1 or frames.stride(1) != W or frames.stride(0) < 0):
        frames = frames.contiguous()
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    elif mask.dtype != torch.uint8:
        mask = (mask != 0).view(torch.uint8)
    mask = mask.to(frames.device).contiguous()
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=frames.device)
    if B == 0 or H * W == 0:
        return out
    nbytes = load().stf_predict_overlay_scratch_bytes(B, H * W)
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=frames.device)
    with torch.cuda.device(frames.device):
        call("stf_predict_overlay", _p(frames), frames.stride(0), _p(mask), B, H, W, color[0], color[1], color[2],
             alpha, paint, _p(out), _p(scratch), stream())
    return out


def shown_frame(inputs):
    """The frame test.py paints on (:173 then :67-68): ``inputs[:, 0, 0]`` of a 5-D model input,
    ``inputs[:, 0]`` of a 4-D one -- a view, not a copy."""
    if inputs.dim() == 5:
        return inputs[:, 0, 0]
    if inputs.dim() == 4:
        return inputs[:, 0]
    raise ValueError(f"model input must be [B, T, C, H, W] or [B, C, H, W], not {tuple(inputs.shape)}")


def parse_views(tta):
    """The view set of a ``tta`` / ``views`` argument: None for ``None`` / ``False`` (off),
    ``("none", "w", "h", "hw")`` for ``True``, else the given non-empty tuple or list of distinct
    views, in its order."""
    if tta is None or tta is False:
        return None
    if tta is True:
        return ALL_VIEWS
    if not isinstance(tta, (tuple, list)):
        raise ValueError(f"views must be True, None / False or a tuple of views from {ALL_VIEWS}, not {tta!r}")
    views = tuple(tta)
    if not views:
        raise ValueError("the view set is empty")
    for v in views:
        if not isinstance(v, str):
            raise ValueError(f"a view must be a string from {ALL_VIEWS}, not {v!r}")
        if v not in VIEWS:
            raise ValueError(f"unknown view {v!r} (one of {ALL_VIEWS})")
    if len(set(views)) != len(views):
        raise ValueError(f"the view set repeats a view: {views}")
    return views


def _check_view(view):
    if not isinstance(view, str) or view not in VIEWS:
        raise ValueError(f"unknown view {view!r} (one of {ALL_VIEWS})")
    return VIEWS[view]


def flip_planes(x, view):
    """``x`` (fp32 device tensor, at least 2-D; made contiguous first if it is not) with the axes of
    ``view`` reversed in every ``H x W`` plane of its last two dimensions: a new tensor, bit for bit
    ``torch.flip`` (``"w"``: dims (-1,), ``"h"``: (-2,), ``"hw"``: both, ``"none"``: a copy)."""
    code = _check_view(view)
    if x.dim() < 2:
        raise ValueError(f"flip_planes needs at least 2 dimensions, not {tuple(x.shape)}")
    if x.dtype != torch.float32:
        raise ValueError(f"flip_planes takes an fp32 tensor, not {x.dtype}")
    if x.numel() >= MAX_PIXELS:
        raise ValueError(f"flip_planes: the tensor must hold fewer than 2^31 elements, not {x.numel()}")
    _device_only(x, "flip_planes")
    x = x.detach().contiguous()
    y = torch.empty_like(x)
    if x.numel():
        H, W = x.shape[-2:]
        with torch.cuda.device(x.device):
            call("stf_flip_planes", _p(x), x.numel() // (H * W), H, W, code, _p(y), stream())
    return y


def _check_tta_rule(rule):
    if rule not in ("argmax", "sigmoid"):
        raise ValueError(f"test-time augmentation averages the probabilities of rule 'argmax' (softmax) or "
                         f"'sigmoid', not {rule!r}")


def _accumulate(logits, rule, channel, view, acc, first, views_if_last):
    """One ``stf_tta_accumulate`` launch on checked tensors; allocates ``acc`` when it is None."""
    B, K, H, W = logits.shape
    if acc is None:
        acc = torch.empty((B, K if rule == "argmax" else 1, H, W), dtype=torch.float32, device=logits.device)
    if logits.numel():
        with torch.cuda.device(logits.device):
            call("stf_tta_accumulate", _p(logits), B, K, H, W, RULES[rule], channel, VIEWS[view], int(first),
                 views_if_last, _p(acc), stream())
    return acc


def tta_probabilities(model, inputs, views=True, rule="argmax", channel=0):
    """Mean class probabilities of ``model`` over mirrored views of ``inputs`` (``[B, C, H, W]`` or
    ``[B, T, C, H, W]``, already in the model's input format): fp32 ``[B, K, h, w]`` for
    ``rule="argmax"`` (softmax over the K classes), ``[B, 1, h, w]`` for ``rule="sigmoid"`` (the
    sigmoid of ``channel``).

    For every view in order the model runs on the flipped copy, and one pass turns its logits into
    probabilities, un-flips them and adds them to the sum; the pass of the last view divides by the
    number of views.  One ``flip_planes`` launch (none for ``"none"``) and one accumulate launch per
    view around the forwards, a fixed order and no atomics: the same bits from run to run, no host
    synchronisation.  Runs in eval mode under ``no_grad`` and puts the model's training mode back."""
    views = parse_views(views)
    if views is None:
        raise ValueError("tta_probabilities needs a view set (True or a tuple of views)")
    _check_tta_rule(rule)
    _device_only(inputs, "tta_probabilities")
    x = inputs.detach().float()
    was_training = model.training
    model.eval()
    acc = None
    try:
        with torch.no_grad():
            for i, view in enumerate(views):
                z = model(x if view == "none" else flip_planes(x, view))
                if isinstance(z, dict):
                    z = z["out"]
                if z.dim() != 4:
                    raise ValueError(f"logits must be [B, K, H, W], not {tuple(z.shape)}")
                if not 1 <= z.shape[1] <= MAX_CLASSES:
                    raise ValueError(f"1..{MAX_CLASSES} classes are supported, not {z.shape[1]}")
                if not 0 <= channel < z.shape[1]:
                    raise ValueError(f"channel {channel} is outside [0, {z.shape[1]})")
                if z.numel() >= MAX_PIXELS:
                    raise ValueError(f"logits must hold fewer than 2^31 elements, not {z.numel()}")
                z = z.detach().float().contiguous()
                acc = _accumulate(z, rule, channel, view, acc, i == 0, len(views) if i == len(views) - 1 else 0)
    finally:
        model.train(was_training)
    return acc


def _batches(model, data_loader, device, tta, rule, channel, threshold, ignore_index):
    """The head of the inference loops.  Checks ``rule`` against ``tta`` (a ``parse_views`` argument, or
    its result) at once; the generator it returns yields, for every batch of the loader,
    ``(inputs, targets, mask, counts, outputs)``: the preprocessed inputs and the targets (or None) on
    the device, ``predict_masks`` of the forward -- of ``tta_probabilities`` with views -- with its
    counts (None without targets), and what the mask was taken from.  The caller owns eval mode and
    ``no_grad``."""
    if rule not in RULES:
        raise ValueError(f"unknown rule {rule!r} (one of {sorted(RULES)})")
    views = parse_views(tta)
    mask_rule, mask_channel = rule, channel
    if views is not None:
        _check_tta_rule(rule)
        if rule == "sigmoid":                       # the mean probability is one plane: mean > threshold
            mask_rule, mask_channel = "threshold", 0
    from .engine import preprocess_input

    def batches():
        for batch in data_loader:
            inputs, targets = batch if isinstance(batch, (tuple, list)) else (batch, None)
            inputs = preprocess_input(inputs, model).to(device)
            outputs = model(inputs) if views is None else tta_probabilities(model, inputs, views, rule, channel)
            counts = None
            if targets is not None:
                targets = targets.to(device)
                mask, counts = predict_masks(outputs, mask_rule, mask_channel, threshold, target=targets,
                                             ignore_index=ignore_index)
            else:
                mask = predict_masks(outputs, mask_rule, mask_channel, threshold)
            yield inputs, targets, mask, counts, outputs

    return batches()


def _predict(model, data_loader, device, views, keep_probs, rule="argmax", channel=0, threshold=0.5,
             ignore_index=None, output_dir=None, prefix="unet", color=(0, 255, 0), alpha=0.5, paint=1,
             keep_masks=False, boundary=False, spacing=1.0, keep_largest=False, min_size=0, connectivity=8):
    """The loop of ``predict`` (``views`` None) and ``predict_tta`` (``views`` a checked view set) with
    ``predict``'s options."""
    return _predict_loop(model, data_loader, device, views, keep_probs, False, 0.0, rule, channel, threshold,
                         ignore_index, output_dir, prefix, color, alpha, paint, keep_masks, boundary, spacing,
                         keep_largest, min_size, connectivity)


def _predict_loop(model, data_loader, device, views, keep_probs, lesions, lesion_overlap, rule="argmax", channel=0,
                  threshold=0.5, ignore_index=None, output_dir=None, prefix="unet", color=(0, 255, 0), alpha=0.5,
                  paint=1, keep_masks=False, boundary=False, spacing=1.0, keep_largest=False, min_size=0,
                  connectivity=8, curves=False, curve_bins=256, curve_channel=1, froc=False, froc_bins=256,
                  froc_overlap=0.0):
    """``_predict``, the lesion-level figures, the score histograms and the FROC tables (``predict_tta`` hands
    ``lesions`` / ``lesion_overlap``, the three ``curve`` options and the three ``froc`` options over)."""
    batches = _batches(model, data_loader, device, views, rule, channel, threshold, ignore_index)
    froc, froc_bins, froc_overlap = _check_froc(froc, froc_bins, froc_overlap, curve_channel)
    curves, curve_bins, curve_channel = _check_curves(curves, curve_bins, curve_channel)
    color = _check_paint(color, alpha, paint)
    if boundary:
        spacing = _check_spacing(spacing)
    connectivity, min_size = _check_components(connectivity, min_size)
    components = bool(keep_largest) or min_size > 0
    if lesions:
        lesion_overlap, _ = _check_lesions(lesion_overlap)
    if output_dir is not None:
        from PIL import Image
        os.makedirs(output_dir, exist_ok=True)
    model.eval()
    all_counts, all_boundary, all_num, all_lesions, masks, probs, idx = [], [], [], [], [], [], 0
    all_hist, all_froc = [], []
    with torch.no_grad():
        for inputs, targets, mask, counts, outputs in batches:
            if keep_probs:
                probs.append(outputs)
            if curves and targets is not None:             # the raw score, before any component filter
                all_hist.append(_batch_hist(outputs, targets, views, rule, channel, curve_bins, curve_channel,
                                            ignore_index))
            if components:
                mask, counts, num = _filter(mask, targets, None, keep_largest, min_size, connectivity, ignore_index)
                all_num.append(num)
            if targets is not None:
                all_counts.append(counts)
                if boundary:
                    all_boundary.append(boundary_metrics(mask, targets, ignore_index, spacing))
                if lesions:
                    all_lesions.append(_lesions(mask, targets, None, connectivity, lesion_overlap, 0,
                                                ignore_index)[0])
                if froc:                                   # the reported mask against the raw score
                    all_froc.append(_batch_froc(mask, outputs, targets, None, views, rule, channel, curve_channel,
                                                froc_bins, connectivity, froc_overlap, ignore_index))
            if output_dir is not None:
                pics = overlay(shown_frame(inputs), mask, color, alpha, paint).cpu().numpy()
                for j, pic in enumerate(pics):
                    Image.fromarray(pic).save(os.path.join(output_dir, f"{prefix}_{idx + j}.png"))
            if keep_masks:
                masks.append(mask)
            idx += mask.shape[0]
    res = {"num": idx, "dice": None, "iou": None, "mean_dice": None, "mean_iou": None}
    if all_counts:
        dice, iou = image_metrics(torch.cat(all_counts))
        res.update(dice=dice, iou=iou, mean_dice=dice.mean(), mean_iou=iou.mean())
    if boundary:
        for k in ("hd", "hd95", "assd"):
            v = torch.cat([m[k] for m in all_boundary]) if all_boundary else None
            res[k] = v
            res["mean_" + k] = None if v is None else torch.nanmean(v)
        res["num_boundary"] = None if not all_boundary else (~torch.isnan(res["hd"])).sum()
    if components:
        res["num_components"] = torch.cat(all_num).to(torch.int64) if all_num else None
    if lesions:
        res.update(_pooled_lesions(all_lesions, "image"))
    if curves:
        res.update(_curve_result(torch.cat(all_hist) if all_hist else None))
    if froc:
        res.update(_froc_loop_result(all_froc))
    if keep_masks:
        res["masks"] = masks
    if keep_probs:
        res["probs"] = probs
    return res


def predict(model, data_loader, device, rule="argmax", channel=0, threshold=0.5, ignore_index=None,
            output_dir=None, prefix="unet", color=(0, 255, 0), alpha=0.5, paint=1, keep_masks=False,
            boundary=False, spacing=1.0, keep_largest=False, min_size=0, connectivity=8):
    """The inference loop of test.py:146-176 for any batch size.

    The loader yields ``inputs`` or ``(inputs, targets)`` (targets may be None).  Returns a dict:
    ``num`` slices seen and, when targets came, per-image ``dice`` / ``iou`` (float64 device
    tensors in slice order) with their means ``mean_dice`` / ``mean_iou`` (None otherwise).
    With ``output_dir`` every slice is written as ``{prefix}_{idx}.png`` (RGB, ``idx`` the running
    slice index); that is the loop's only device-to-host copy, one per batch.  ``keep_masks=True``
    adds ``masks``, the list of each batch's ``uint8 [B, H, W]`` device mask.
    ``boundary=True`` adds, when targets came, ``boundary_metrics`` of every mask against its target:
    per-image ``hd`` / ``hd95`` / ``assd`` (NaN where the mask or the target is empty), their means
    over the defined images ``mean_hd`` / ``mean_hd95`` / ``mean_assd`` (NaN when there is none) and
    ``num_boundary``, the number of defined images -- all device tensors, no host synchronisation.
    ``keep_largest=True`` and / or ``min_size > 0`` clean every batch's mask with
    ``filter_components`` (at ``connectivity``) before anything consumes it: ``dice`` / ``iou`` come
    from the filter's counts, and the boundary metrics, the overlays and ``masks`` see the filtered
    mask.  The result then gains ``num_components``, an int64 device tensor in slice order: the
    components of each mask before filtering.  No device-to-host copy is added.  With both options
    off nothing of this runs and the result has no such key.
    ``predict_tta`` is this loop with mirror test-time augmentation and, with or without it, the
    lesion-level detection figures (``lesions=True``)."""
    return _predict(model, data_loader, device, None, False, rule, channel, threshold, ignore_index, output_dir,
                    prefix, color, alpha, paint, keep_masks, boundary, spacing, keep_largest, min_size, connectivity)


def predict_volumes(model, data_loader, device, depths, *, tta=None, rule="argmax", channel=0, threshold=0.5,
                    ignore_index=None, keep_largest=False, min_size=0, connectivity=26, keep_masks=False,
                    boundary=False, spacing=1.0, lesions=False, lesion_overlap=0.0, curves=False, curve_bins=256,
                    curve_channel=1, froc=False, froc_bins=256, froc_overlap=0.0):
    """The inference loop over volumes: the loader yields slices in volume order -- ``depths[0]``
    slices of volume 0, then volume 1 and so on (``stfunet.dataset.volume_order`` puts a
    ``DriveDataset`` into that order); batches may straddle volume boundaries.

    Every batch gets a forward (``tta_probabilities`` when ``tta`` is set, as in ``predict_tta``) and
    ``predict_masks``.  With ``keep_largest=True`` and / or ``min_size > 0`` the masks and targets
    are held on the device until their volume is complete; all volumes a batch completes are cleaned
    by one ``filter_components_3d`` call (at ``connectivity``, ``min_size`` in voxels), so the memory
    held is bounded by the largest volume plus one batch.  With both options off no labelling kernel
    runs and the per-volume counts are the per-slice counts summed by volume on the device.

    Returns a dict of device tensors in volume order, with no host synchronisation in the loop:
    ``num`` slices seen, ``num_volumes``, per-volume ``dice`` / ``iou`` (from the counts summed over
    the volume's slices: the per-case numbers) with ``mean_dice`` / ``mean_iou`` over the volumes
    (all None without targets), ``num_components`` (int64 ``[V]``, the components of each volume
    before filtering; only with a component option on) and, with ``keep_masks``, ``masks``, a list
    of ``V`` ``uint8 [D_v, H, W]`` masks.  Raises ``ValueError`` when the loader's slice total is not
    ``sum(depths)``.

    ``boundary=True`` adds, when targets came, ``boundary_metrics_3d`` of every volume's mask (after
    the component filter, when one is on) against its target at ``spacing`` (a number, a triple
    ``(sz, sy, sx)`` or one triple per volume): per-volume ``hd`` / ``hd95`` / ``assd`` (NaN where the
    mask or the target is empty), their means over the defined volumes ``mean_hd`` / ``mean_hd95`` /
    ``mean_assd`` (NaN when there is none) and ``num_boundary``, the number of defined volumes; all
    None without targets.  The slices are then held until their volume is complete, as for the
    component options; with those off still no labelling kernel runs.  Without ``boundary`` nothing
    of this runs and the result has no such key.

    ``lesions=True`` adds, when targets came, ``lesion_metrics_3d`` of every volume's mask (after the
    component filter, when one is on) against its target at ``connectivity`` and
    ``min_overlap=lesion_overlap``, one call per flush: ``lesion_counts`` int64 ``[V, 4]`` = (n_target,
    matched_target, n_pred, matched_pred) per case, the pooled ``lesion_sensitivity`` = sum
    matched_target / sum n_target and ``lesion_precision`` = sum matched_pred / sum n_pred,
    ``false_findings`` = n_pred - matched_pred per case and their mean ``false_findings_per_case``; all
    None without targets.  The slices are held until their volume is complete, as for ``boundary``.
    With the default ``lesions=False`` nothing of this runs and the result has no such key.

    ``curves=True`` adds, when targets came, the threshold-free figures of the raw scores (before any
    component filter), one ``stf_score_hist`` launch per batch at ``curve_bins`` and no held slices: the
    keys of ``predict_tta``'s ``curves=True``, per case instead of per image.  Without the flag nothing of
    this runs and the result has no such key.

    ``froc=True`` adds, when targets came, ``lesion_scores_3d`` of every volume's mask (after the component
    filter, when one is on) against its target and the score ``curves=True`` uses (``curve_channel``), at
    ``connectivity``, ``bins=froc_bins`` and ``min_overlap=froc_overlap``, one ``stf_froc3d`` call per flush: the
    keys of ``predict_tta``'s ``froc=True``, per case instead of per image.  The slices' scores are held with
    their masks until the volume is complete.  Without the flag nothing of this runs and the result has no
    such key.

    Not here: overlays (``keep_masks=True`` and ``overlay`` cover them) and anisotropic connectivity."""
    batches = _batches(model, data_loader, device, tta, rule, channel, threshold, ignore_index)
    connectivity, min_size = _check_components_3d(connectivity, min_size)
    if depths is None:
        raise ValueError("depths must be a sequence of positive integers, one per volume, not None")
    depths = _check_depths(depths)
    components = bool(keep_largest) or min_size > 0
    V, total = len(depths), sum(depths)
    rows = _check_spacing_3d(spacing, V) if boundary else None
    if lesions:
        lesion_overlap, _ = _check_lesions(lesion_overlap)
    froc, froc_bins, froc_overlap = _check_froc(froc, froc_bins, froc_overlap, curve_channel)
    curves, curve_bins, curve_channel = _check_curves(curves, curve_bins, curve_channel)
    views = parse_views(tta)
    model.eval()
    slice_volume = torch.repeat_interleave(torch.arange(V), torch.tensor(depths, dtype=torch.int64)).to(device)
    vol_counts = None                               # options off: int64 [V, 3], summed as the slices come
    vol_hist = None                                 # curves: int64 [V, 2, bins + 1], summed as the slices come
    held_masks, held_targets, held, done = [], [], 0, 0   # options on: slices of volumes not yet complete
    held_scores, all_froc = [], []                  # froc: the slices' scores, held like their masks
    all_counts, all_num, all_boundary, all_lesions, masks, idx, with_targets = [], [], [], [], [], 0, None
    with torch.no_grad():
        for _, targets, mask, counts, outputs in batches:
            if with_targets is None:
                with_targets = targets is not None
            elif with_targets != (targets is not None):
                raise ValueError("the loader yields targets for some batches and none for others")
            B = mask.shape[0]
            if idx + B > total:
                raise ValueError(f"the loader yields more than the {total} slices of depths")
            if curves and targets is not None:
                hist = _batch_hist(outputs, targets, views, rule, channel, curve_bins, curve_channel, ignore_index)
                if vol_hist is None:
                    vol_hist = torch.zeros((V,) + tuple(hist.shape[1:]), dtype=torch.int64, device=hist.device)
                vol_hist.index_add_(0, slice_volume[idx:idx + B], hist)
            if not components:
                if targets is not None:
                    if vol_counts is None:
                        vol_counts = torch.zeros((V, 3), dtype=torch.int64, device=counts.device)
                    vol_counts.index_add_(0, slice_volume[idx:idx + B], counts)
                if keep_masks:
                    masks.append(mask)
            if components or ((boundary or lesions or froc) and targets is not None):
                held_masks.append(mask)
                if targets is not None:
                    held_targets.append(targets)
                    if froc:
                        held_scores.append(outputs["out"] if isinstance(outputs, dict) else outputs)
                held += B
                k = take = 0                         # the volumes this batch completes, and their slices
                while done + k < V and take + depths[done + k] <= held:
                    take += depths[done + k]
                    k += 1
                if k:
                    m = torch.cat(held_masks) if len(held_masks) > 1 else held_masks[0]
                    t = None
                    if targets is not None:
                        t = torch.cat(held_targets) if len(held_targets) > 1 else held_targets[0]
                    out = m[:take]
                    if components:
                        out, counts, num = _filter(out, None if t is None else t[:take], depths[done:done + k],
                                                   keep_largest, min_size, connectivity, ignore_index)
                        all_num.append(num)
                        if counts is not None:
                            all_counts.append(counts)
                        if keep_masks:
                            masks.extend(out.split(depths[done:done + k]))
                    if boundary and t is not None:
                        all_boundary.append(_boundary3d(out.contiguous(), t[:take], depths[done:done + k],
                                                        rows[done:done + k], ignore_index)[0])
                    if lesions and t is not None:
                        all_lesions.append(_lesions(out.contiguous(), t[:take], depths[done:done + k], connectivity,
                                                    lesion_overlap, 0, ignore_index)[0])
                    if froc and t is not None:
                        sc = torch.cat(held_scores) if len(held_scores) > 1 else held_scores[0]
                        all_froc.append(_batch_froc(out.contiguous(), sc[:take], t[:take], depths[done:done + k], views,
                                                    rule, channel, curve_channel, froc_bins, connectivity,
                                                    froc_overlap, ignore_index))
                        held_scores = [sc[take:]] if take < held else []
                    held_masks = [m[take:]] if take < held else []
                    held_targets = [t[take:]] if t is not None and take < held else []
                    held -= take
                    done += k
            idx += B
    if idx != total:
        raise ValueError(f"the loader yielded {idx} slices, but depths sum to {total}")
    res = {"num": idx, "num_volumes": V, "dice": None, "iou": None, "mean_dice": None, "mean_iou": None}
    if not components and keep_masks:
        masks = list(torch.cat(masks).split(depths)) if masks else []
    if components and all_counts:
        vol_counts = torch.cat(all_counts)
    if vol_counts is not None:
        dice, iou = image_metrics(vol_counts)
        res.update(dice=dice, iou=iou, mean_dice=dice.mean(), mean_iou=iou.mean())
    if boundary:
        per_volume = torch.cat(all_boundary) if all_boundary else None
        for j, k in enumerate(("hd", "hd95", "assd")):
            v = None if per_volume is None else per_volume[:, j]
            res[k] = v
            res["mean_" + k] = None if v is None else torch.nanmean(v)
        res["num_boundary"] = None if per_volume is None else (~torch.isnan(per_volume[:, 0])).sum()
    if components:
        res["num_components"] = torch.cat(all_num).to(torch.int64) if all_num else None
    if lesions:
        res.update(_pooled_lesions(all_lesions, "case"))
    if curves:
        res.update(_curve_result(vol_hist))
    if froc:
        res.update(_froc_loop_result(all_froc))
    if keep_masks:
        res["masks"] = masks
    return res


def predict_tta(model, data_loader, device, tta=True, keep_probs=False, **options):
    """``predict`` with mirror test-time augmentation: ``options`` are ``predict``'s keywords and the two
    of the lesion-level figures, ``lesions=False`` and ``lesion_overlap=0.0``.

    Each batch's mask comes from ``tta_probabilities(model, inputs, tta, rule, channel)``: its
    first maximum over the classes for ``rule="argmax"``, ``mean > threshold`` for ``rule="sigmoid"``
    (``predict_masks``' rule ``"threshold"``).  Counts, ``ignore_index``, the component filter, the
    boundary metrics, the lesion metrics, the overlays (painted on the un-flipped frame) and ``keep_masks`` see that mask
    as ``predict``'s see the plain one.  ``tta``: ``True`` for ``("none", "w", "h", "hw")`` or a
    non-empty tuple of distinct views, applied in the order given; ``None`` / ``False`` is plain
    ``predict``, which then runs nothing of this.  ``keep_probs=True`` (only with ``tta`` on) adds
    ``probs``, the list of each batch's mean probabilities.

    ``lesions=True`` adds, when targets came, the lesion-level detection figures of every mask (after
    the component filter, when one is on) against its target, one ``lesion_metrics`` launch sequence per
    batch at ``connectivity`` and ``min_overlap=lesion_overlap``: ``lesion_counts`` int64 ``[num, 4]`` =
    (n_target, matched_target, n_pred, matched_pred) per image, the pooled ``lesion_sensitivity`` =
    sum matched_target / sum n_target and ``lesion_precision`` = sum matched_pred / sum n_pred (NaN
    without lesions / components), ``false_findings`` = n_pred - matched_pred per image and their mean
    ``false_findings_per_image``; all None without targets.  Device tensors, no host synchronisation;
    with the default ``lesions=False`` nothing of this runs and the result has no such key.  It works
    with ``tta=None`` too: ``predict_tta(model, loader, device, tta=None, lesions=True)`` is the plain
    loop with the lesion figures (``predict``'s own parameter list is pinned and does not take them).

    ``curves=True`` (with ``curve_bins=256`` and ``curve_channel=1``; with or without ``tta``) adds, when
    targets came, the threshold-free figures of the raw scores, before ``keep_largest`` / ``min_size``: one
    ``stf_score_hist`` launch per batch on what the batch's mask was taken from.  The score is, for
    ``rule="argmax"``, the softmax probability of class ``curve_channel`` (the mean probability under
    ``tta``); for ``rule="sigmoid"`` the sigmoid of the rule's own plane ``channel`` (its mean under ``tta``);
    for ``rule="threshold"`` plane ``channel`` as it is.  The result gains ``score_hist`` int64
    ``[num, 2, curve_bins + 1]`` (``score_histogram`` per image), ``curves`` = ``threshold_curves`` of the
    histogram pooled over all images, ``case_auroc`` / ``case_average_precision`` per image (NaN where a
    side is empty), ``mean_case_dice_curve`` = the mean over images of each image's Dice at every
    threshold and ``best_case_threshold``, its first maximum; all None without targets.  Device tensors,
    no host synchronisation; without the flag nothing of this runs and the result has no such key.

    ``froc=True`` (with ``froc_bins=256`` and ``froc_overlap=0.0``; with or without ``tta``) adds, when targets
    came, ``lesion_scores`` of every reported mask (after ``keep_largest`` / ``min_size``) against its target and
    the score ``curves=True`` uses (``curve_channel``; the mean probability under ``tta``), at ``connectivity``,
    ``bins=froc_bins`` and ``min_overlap=froc_overlap``, one ``stf_froc`` call per batch.  The result gains
    ``froc_hist`` int64 ``[num, 3, froc_bins + 1]`` per image, ``froc`` = ``froc_curves`` of the table pooled over
    all images with ``cases`` = their number, and ``lesion_scores`` int64 ``[num, 2, 64, 3]``, the (area, hit,
    score) tables; all None without targets.  Device tensors, no host synchronisation; without the flag
    nothing of this runs and the result has no such key."""
    views = parse_views(tta)
    if keep_probs and views is None:
        raise ValueError("keep_probs needs test-time augmentation (tta)")
    lesions, lesion_overlap = options.pop("lesions", False), options.pop("lesion_overlap", 0.0)
    if views is None and not lesions and not options.get("curves") and not options.get("froc"):
        for k in ("curves", "curve_bins", "curve_channel", "froc", "froc_bins", "froc_overlap"):
            options.pop(k, None)
        return predict(model, data_loader, device, **options)
    return _predict_loop(model, data_loader, device, views, bool(keep_probs), lesions, lesion_overlap, **options)
