"""torch / numpy restatement of the inference outputs (tests only).

    mask     argmax:  first maximum over the classes, a NaN wins      (torch.argmax)
             sigmoid: torch.sigmoid(logits[:, channel]) > threshold   (fp32)
    counts   per image (|P & T|, |P|, |T|), P = mask > 0, T = target > 0, over the pixels whose
             target differs from ``ignore`` (all of them when it is None)
    metrics  dice = (2I + s) / (P + T + s),  iou = (I + s) / (P + T - I + s),  float64
    overlay  gray = uint8(((x - min) / (max - min + 1e-8)) * 255) per image, every operation in
             fp32; painted pixels ((mask != 0) == paint) uint8(gray * (1 - alpha) + colour_c * alpha),
             the others gray in all three channels

``tests/golden/predict.npz`` (make_golden_predict.py, the reference's own functions) pins it;
the GPU tests use it for shapes the fixture does not hold.
"""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def mask_ref(logits, rule="argmax", channel=0, threshold=0.5):
    logits = logits.detach().float().cpu()
    if rule == "argmax":
        return logits.argmax(1).to(torch.uint8)
    return (torch.sigmoid(logits[:, channel]) > threshold).to(torch.uint8)


def counts_ref(mask, target, ignore=None):
    mask, target = mask.cpu(), target.cpu()
    keep = torch.ones_like(target, dtype=torch.bool) if ignore is None else target != ignore
    p, t = (mask > 0) & keep, (target > 0) & keep
    return torch.stack([(p & t).flatten(1).sum(1), p.flatten(1).sum(1), t.flatten(1).sum(1)], 1)


def metrics_ref(counts, smooth=1e-5):
    i, p, t = counts.cpu().double().unbind(1)
    return (2 * i + smooth) / (p + t + smooth), (i + smooth) / (p + t - i + smooth)


def overlay_ref(frames, mask, color=(0, 255, 0), alpha=0.5, paint=1):
    frames, mask = frames.detach().float().cpu().numpy(), mask.cpu().numpy()
    f32 = np.float32
    a = f32(alpha)
    oma = f32(1) - a
    out = np.empty(frames.shape + (3,), dtype=np.uint8)
    for b, x in enumerate(frames):
        mn, mx = x.min(), x.max()
        gray = (((x - mn) / ((mx - mn) + f32(1e-8))) * f32(255)).astype(np.uint8)
        painted = (mask[b] != 0) == bool(paint)
        for c in range(3):
            v = gray.astype(f32) * oma + f32(color[c]) * a
            assert v.dtype == f32
            out[b, :, :, c] = np.where(painted, v.astype(np.uint8), gray)
    return torch.from_numpy(out)


def fixture_cases():
    """The reference-generated cases of tests/golden/predict.npz as dicts of tensors / scalars."""
    g = np.load(os.path.join(GOLDEN, "predict.npz"))
    out = []
    for name in g["names"].tolist():
        src = str(g[name + ".inputs"])
        c = dict(name=name, rule=str(g[name + ".rule"]), channel=int(g[name + ".channel"]),
                 threshold=float(g[name + ".threshold"]), color=tuple(int(v) for v in g[name + ".color"]),
                 alpha=float(g[name + ".alpha"]), paint=int(g[name + ".paint"]))
        for k in ("logits", "target", "frames"):
            c[k] = torch.from_numpy(g[f"{src}.{k}"])
        for k in ("mask", "counts", "dice", "iou", "overlay"):
            c[k] = torch.from_numpy(g[f"{name}.{k}"])
        if name + ".counts_ign255" in g.files:
            for k in ("counts", "dice", "iou"):
                c[k + "_ign255"] = torch.from_numpy(g[f"{name}.{k}_ign255"])
        out.append(c)
    return out


def away_from_ties(logits, rule="argmax", channel=0, threshold=0.5, margin=1e-3):
    """``logits`` with every pixel moved at least ``margin`` away from a tie: class logits of a
    pixel pairwise ``margin`` apart (argmax), the channel's logit ``margin`` away from
    logit(threshold) (sigmoid; |d sigmoid / dx| <= 1/4, ulps of expf are ~1e-7).  The device's expf
    and the host's differ by ulps; this is a condition on the inputs, no pixel is left out."""
    x = logits.clone()
    if rule == "sigmoid":
        edge = float(np.log(threshold / (1 - threshold)))
        d = x[:, channel] - edge
        x[:, channel] = edge + torch.where(d.abs() < margin, torch.where(d < 0, -margin, margin).to(d.dtype), d)
        return x
    K = x.shape[1]
    order = x.argsort(1)
    ranks = order.argsort(1).to(x.dtype)
    x = x + ranks * margin                      # keeps the order, widens every gap by >= margin
    assert K == 1 or (x.sort(1).values.diff(dim=1) >= margin * 0.99).all()
    return x
