"""Inference outputs at cfg2's output (64 x 2 x 256^2 logits, the shown frame a strided view of the
64 x 8 x 256^2 input): mask + per-image counts + Dice / IoU + overlay on the gfx950 kernels
(stfunet.predict, csrc/predict.hip) against the same results from the torch op sequence of the
reference's test.py:168-169, :71, merge_images and compute_metrics on the same GPU tensors --
once vectorised over the batch and once slice by slice, as the reference's batch-size-1 loop runs it.

The three are timed in turn inside every round (interleaved, same process), with device events
around ``--iters`` calls; the median round is reported.  Bytes: ``algorithmic`` counts every input
and output once (logits, int64 target, frame, mask, overlay); ``moved`` adds what the two-launch
overlay reads again (the frame for the blend after the min / max pass, the mask).  Prints one JSON
line.

    python tools/bench_predict.py [--rule argmax|sigmoid] [--batch 64] [--size 256] [--rounds 7] [--iters 20]
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "stf-unet_amd")]
import torch  # noqa: E402

from stfunet import image_metrics, overlay, predict_masks  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rule", default="argmax", choices=["argmax", "sigmoid"])
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_predict.py measures on the GPU: no ROCm device found")

B, K, H, W = args.batch, 2, args.size, args.size
COLOR, ALPHA, PAINT, SMOOTH = (0, 255, 0), 0.5, 0, 1e-5
torch.manual_seed(0)
logits = torch.randn(B, K, H, W, device="cuda") * 2
target = (torch.rand(B, H, W, device="cuda") < 0.3).long()
inputs = torch.randn(B, 8, H, W, device="cuda")
frames = inputs[:, 0]                                   # the shown frame: a view, batch stride 8 * H * W
color_t = torch.tensor(COLOR, dtype=torch.float32, device="cuda")


def device_path():
    mask, counts = predict_masks(logits, args.rule, 0, 0.5, target=target)
    dice, iou = image_metrics(counts, SMOOTH)
    return mask, dice, iou, overlay(frames, mask, COLOR, ALPHA, PAINT)


def _torch_slices(x, t, f):
    """test.py:168-169 / train_and_eval.py:331, compute_metrics, test.py:71-76 and merge_images on
    device tensors with a leading batch dimension (1 for the slice-by-slice run)."""
    if args.rule == "sigmoid":
        pred = torch.sigmoid(x[:, 0]) > 0.5
    else:
        pred = x.argmax(1) > 0
    tb = t > 0
    inter = (pred & tb).flatten(1).sum(1).double()
    p, g = pred.flatten(1).sum(1).double(), tb.flatten(1).sum(1).double()
    dice = (2 * inter + SMOOTH) / (p + g + SMOOTH)
    iou = (inter + SMOOTH) / (p + g - inter + SMOOTH)
    mn, mx = f.amin((1, 2), keepdim=True), f.amax((1, 2), keepdim=True)
    gray = ((f - mn) / (mx - mn + 1e-8) * 255).to(torch.uint8)
    painted = pred == bool(PAINT)
    blend = (gray.float().unsqueeze(-1) * (1 - ALPHA) + color_t * ALPHA).to(torch.uint8)
    pic = torch.where(painted.unsqueeze(-1), blend, gray.unsqueeze(-1).expand(-1, -1, -1, 3))
    return pred.to(torch.uint8), dice, iou, pic


def torch_batched():
    return _torch_slices(logits, target, frames)


def torch_per_slice():
    out = [_torch_slices(logits[b:b + 1], target[b:b + 1], frames[b:b + 1]) for b in range(B)]
    return tuple(torch.cat(v) for v in zip(*out))


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters           # us per call


paths = (("device", device_path, args.iters), ("torch_batched", torch_batched, args.iters),
         ("torch_per_slice", torch_per_slice, max(1, args.iters // 10)))
for _, fn, _ in paths:                                  # warm-up: code objects, allocator
    for _ in range(3):
        fn()
torch.cuda.synchronize()
us = {name: [] for name, _, _ in paths}
for _ in range(args.rounds):
    for name, fn, iters in paths:
        us[name].append(timed(fn, iters))

ref, got = torch_batched(), device_path()
if args.rule == "argmax":
    same_mask = int(((got[0] > 0) != (ref[0] > 0)).sum())
else:
    same_mask = int((got[0] != ref[0]).sum())
HW = H * W
algorithmic = B * HW * ((K if args.rule == "argmax" else 1) * 4 + 8 + 4 + 1 + 3) + B * 24
moved = algorithmic + B * HW * (4 + 1)
med = {k: statistics.median(v) for k, v in us.items()}
print(json.dumps({
    "tool": "bench_predict", "rule": args.rule, "shape": [B, K, H, W], "rounds": args.rounds, "iters": args.iters,
    "us_per_batch": {k: round(v, 1) for k, v in med.items()},
    "us_min_max": {k: [round(min(v), 1), round(max(v), 1)] for k, v in us.items()},
    "speedup_vs_torch_batched": round(med["torch_batched"] / med["device"], 2),
    "speedup_vs_torch_per_slice": round(med["torch_per_slice"] / med["device"], 2),
    "algorithmic_bytes": algorithmic, "moved_bytes": moved,
    "algorithmic_TBps": round(algorithmic / med["device"] / 1e6, 3),
    "moved_TBps": round(moved / med["device"] / 1e6, 3),
    "mask_pixels_differing_from_torch": same_mask,
    "overlay_bytes_differing_from_torch": int((got[3] != ref[3]).sum()),
    "max_abs_dice_difference": float((got[1] - ref[1]).abs().max()),
}))
