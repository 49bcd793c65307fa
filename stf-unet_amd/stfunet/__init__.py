"""MI355X-native (gfx950) STF-Unet training hot path.

Drop-in replacements for the reference's ``src.UNet`` / ``src.STFLSTMUNet``
(same constructor signatures, ``input_format`` attribute, ``{"out": logits}``
output and ``state_dict`` keys) whose forward/backward run hand-written HIP
kernels through the C ABI in ``include/stfunet.h``.
"""
from . import _lib  # noqa: F401
from . import predict  # noqa: F401  (the module; its loop is stfunet.predict.predict)
from .ema import WeightEMA  # noqa: F401
from .loss import boundary_criterion, boundary_loss, criterion, signed_distance_maps  # noqa: F401
from .optim import clip_grad_norm_  # noqa: F401
from .predict import (boundary_metrics, boundary_metrics_3d, connected_components,  # noqa: F401
                      connected_components_3d, distance_transform_3d, distance_transform_sq, filter_components,
                      filter_components_3d, flip_planes, froc_curves, image_metrics, lesion_metrics,
                      lesion_metrics_3d, lesion_scores, lesion_scores_3d, overlay, predict_masks, predict_tta,
                      predict_volumes, score_histogram, threshold_curves, tta_probabilities)
from .resize import upsample_logits  # noqa: F401
from .stf_lstm_unet import STFLSTMUNet  # noqa: F401
from .unet import UNet  # noqa: F401

__all__ = ["STFLSTMUNet", "UNet", "WeightEMA", "boundary_criterion", "boundary_loss", "boundary_metrics",
           "boundary_metrics_3d", "clip_grad_norm_",
           "connected_components", "connected_components_3d", "criterion", "distance_transform_3d",
           "distance_transform_sq", "filter_components", "filter_components_3d", "flip_planes", "froc_curves",
           "image_metrics", "lesion_metrics", "lesion_metrics_3d", "lesion_scores", "lesion_scores_3d",
           "overlay", "predict", "predict_masks", "predict_tta", "predict_volumes", "score_histogram",
           "signed_distance_maps", "threshold_curves", "tta_probabilities", "upsample_logits"]
