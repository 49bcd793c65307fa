"""Generate tests/golden/predict.npz by running the REFERENCE's inference helpers on the CPU.

    python tests/golden/make_golden_predict.py  [--ref /root/reference]

Called from the reference, imported by path under a synthetic ``train_utils`` package:

* ``compute_metrics`` (train_utils/visualize.py:9-50): per-image Dice and IoU;
* ``merge_images`` (train_utils/merge_tumor_images.py:94-120) in its ``border_only=False`` path
  with a 3-channel image, which is pure numpy.

Both modules import ``cv2`` / ``torchvision`` at the top; where one of those is not installed an
empty stub module stands in for the name (nothing of a stub is ever called).

Restated here, because they sit inside functions that need a dataset or cv2:

* test.py:168-169  ``probs = torch.sigmoid(outputs); preds = (probs > 0.5)``, of channel 0
  (:172) -- with the threshold and the channel as parameters;
* train_and_eval.py:331  ``output.argmax(1)``, the prediction ``evaluate`` scores;
* test.py:71  ``((raw - raw.min()) / (raw.max() - raw.min() + 1e-8) * 255).astype(np.uint8)``;
* test.py:72  GRAY2BGR = the gray plane in all three channels;
* test.py:75-76  ``mask = (pred > 0.5) * 255; mask = 255 - mask`` (the inversion is ``paint=0``).

The device's expf differs from the host's by ulps, so the generator asserts a condition on the
INPUTS: no random logit's probability lies within 1e-4 of its threshold and no two class logits
of a pixel lie within 1e-4 of each other.  Planted specials (exact 0.0, +-inf, +-80, NaN, exact
ties) are exact by construction and exempt.  No pixel is left out of any comparison.

Each case ``<name>.*`` stores logits, target, frames (under the case ``<name>.inputs`` names:
two cases share their inputs), rule, channel, threshold, color, alpha,
paint and the expected mask, counts [B][3] = (|P&T|, |P|, |T|), dice, iou, overlay
[B][H][W][3].  Case ``pad255`` also stores counts / dice / iou with its 255-valued target
pixels dropped (``*_ign255``: the reference called on the kept pixels only).  ``names`` lists
the cases.  The archive is written with fixed timestamps, so a rerun reproduces it byte for byte.
"""
import argparse
import importlib
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
MARGIN = 1e-4


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference(ref):
    for name in ("cv2", "torchvision", "torchvision.transforms", "torchvision.transforms.functional", "tqdm"):
        try:
            importlib.import_module(name)
        except ImportError:
            stub = types.ModuleType(name)
            if name == "tqdm":
                stub.tqdm = None
            sys.modules[name] = stub
            parent, _, child = name.rpartition(".")
            if parent:
                setattr(sys.modules[parent], child, stub)
    pkg = types.ModuleType("train_utils")
    pkg.__path__ = [os.path.join(ref, "train_utils")]
    sys.modules["train_utils"] = pkg
    vis = _load(os.path.join(ref, "train_utils/visualize.py"), "train_utils.visualize")
    mti = _load(os.path.join(ref, "train_utils/merge_tumor_images.py"), "train_utils.merge_tumor_images")
    return vis.compute_metrics, mti.merge_images


def check_margins(logits, rule, channel, threshold, planted):
    """The input condition of the module docstring, on every pixel that is not planted."""
    free = ~planted
    if rule == "sigmoid":
        p = torch.sigmoid(logits[:, channel].double())
        assert ((p - threshold).abs()[free] >= MARGIN).all(), "a probability within 1e-4 of the threshold"
    else:
        K = logits.shape[1]
        for a in range(K):
            for b in range(a + 1, K):
                d = (logits[:, a].double() - logits[:, b].double()).abs()
                assert (d[free] >= MARGIN).all(), "two class logits within 1e-4"


def expected(compute_metrics, merge_images, c):
    logits, target, frames = c["logits"], c["target"], c["frames"]
    rule, ch, thr = c["rule"], c["channel"], c["threshold"]
    if rule == "sigmoid":
        probs = torch.sigmoid(logits)                       # test.py:168
        mask = (probs > thr)[:, ch].to(torch.uint8)         # :169, :172
    else:
        mask = logits.argmax(1).to(torch.uint8)             # train_and_eval.py:331
    B = logits.shape[0]
    counts, dice, iou, pics = [], [], [], []
    for b in range(B):
        if rule == "sigmoid":
            d, i = compute_metrics(logits[b, ch], target[b], threshold=thr, apply_sigmoid=True)
        else:
            d, i = compute_metrics(mask[b].float(), target[b], threshold=0.5, apply_sigmoid=False)
        dice.append(float(d))
        iou.append(float(i))
        p, t = mask[b] > 0, target[b] > 0.5
        counts.append([int((p & t).sum()), int(p.sum()), int(t.sum())])
        raw_np = frames[b].numpy()
        raw_np = ((raw_np - raw_np.min()) / (raw_np.max() - raw_np.min() + 1e-8) * 255).astype(np.uint8)   # :71
        raw_img = np.stack([raw_np] * 3, axis=-1)                                                           # :72
        mask_np = (mask[b].numpy() > 0.5).astype(np.uint8) * 255                                            # :75
        if c["paint"] == 0:
            mask_np = 255 - mask_np                                                                         # :76
        pics.append(merge_images(raw_img, mask_np, tuple(c["color"]), alpha=c["alpha"]))
    out = {"mask": mask.numpy(), "counts": np.array(counts, dtype=np.int64),
           "dice": np.array(dice, dtype=np.float64), "iou": np.array(iou, dtype=np.float64),
           "overlay": np.stack(pics)}
    if c.get("ignore") is not None:
        cs, ds, is_ = [], [], []
        for b in range(B):
            keep = target[b] != c["ignore"]
            if rule == "sigmoid":
                d, i = compute_metrics(logits[b, ch][keep], target[b][keep], threshold=thr, apply_sigmoid=True)
            else:
                d, i = compute_metrics(mask[b][keep].float(), target[b][keep], threshold=0.5, apply_sigmoid=False)
            p, t = (mask[b] > 0)[keep], (target[b] > 0.5)[keep]
            cs.append([int((p & t).sum()), int(p.sum()), int(t.sum())])
            ds.append(float(d))
            is_.append(float(i))
        tag = f"_ign{c['ignore']}"
        out.update({"counts" + tag: np.array(cs, dtype=np.int64), "dice" + tag: np.array(ds, dtype=np.float64),
                    "iou" + tag: np.array(is_, dtype=np.float64)})
    return out


def cases():
    def rnd(seed, *shape, scale=2.0):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale

    def tgt(seed, B, H, W, hi=2):
        return torch.randint(0, hi, (B, H, W), generator=torch.Generator().manual_seed(seed))

    def case(name, logits, target, frames, rule, channel=0, threshold=0.5, color=(0, 255, 0), alpha=0.5, paint=1,
             planted=None, ignore=None, inputs_of=None):
        planted = torch.zeros(logits[:, 0].shape, dtype=torch.bool) if planted is None else planted
        check_margins(logits, rule, channel, threshold, planted)
        return dict(name=name, logits=logits, target=target, frames=frames, rule=rule, channel=channel,
                    threshold=threshold, color=color, alpha=alpha, paint=paint, ignore=ignore, inputs_of=inputs_of or name)

    out = []
    # 1x1 images (a one-pixel frame is constant: gray 0), K = 1
    out.append(case("one_px", torch.tensor([1.5, -0.75]).reshape(2, 1, 1, 1), torch.tensor([1, 1]).reshape(2, 1, 1),
                    torch.tensor([3.25, -1.0]).reshape(2, 1, 1), "sigmoid"))
    # HW = 15: the image bases after the first are not 16-byte aligned
    out.append(case("odd_argmax", rnd(11, 3, 2, 3, 5), tgt(12, 3, 3, 5), rnd(13, 3, 3, 5, scale=1.0), "argmax",
                    alpha=0.37))
    out.append(case("odd_sigmoid_k4", rnd(21, 3, 4, 3, 5), tgt(22, 3, 3, 5), rnd(23, 3, 3, 5, scale=1.0).abs(),
                    "sigmoid", channel=3, threshold=0.3, alpha=1.0, paint=0, color=(255, 0, 128)))
    # planted specials, the test.py recipe (sigmoid of channel 0, threshold 0.5, inverted mask)
    lg = rnd(31, 2, 2, 17, 19)
    planted = torch.zeros(2, 17, 19, dtype=torch.bool)
    inf, nan = float("inf"), float("nan")
    for i, (v0, v1) in enumerate([(0.0, 1.0), (-0.0, -1.0), (inf, 0.0), (-inf, 0.0), (80.0, -80.0), (-80.0, 80.0),
                                  (nan, 0.0), (0.0, nan), (nan, nan), (inf, inf), (-inf, -inf), (2.5, 2.5),
                                  (0.0, 0.0), (-inf, nan), (inf, nan)]):
        for b in range(2):
            y, x = (5 * i + 3 * b) % 17, (7 * i + b) % 19
            lg[b, 0, y, x], lg[b, 1, y, x] = v0, v1
            planted[b, y, x] = True
    fr = rnd(33, 2, 17, 19, scale=1.0)
    out.append(case("specials_sigmoid", lg, tgt(32, 2, 17, 19), fr, "sigmoid", paint=0, planted=planted))
    out.append(case("specials_argmax", lg, tgt(32, 2, 17, 19), fr, "argmax", alpha=0.0, planted=planted,
                    inputs_of="specials_sigmoid"))
    # all-background target with an all-background prediction (dice = iou = 1); image 1's frame constant
    mag = rnd(41, 2, 8, 12).abs() + 1.0
    fr = rnd(43, 2, 8, 12, scale=1.0)
    fr[1] = -2.5
    out.append(case("all_background", torch.stack([mag, -mag], 1), torch.zeros(2, 8, 12, dtype=torch.int64), fr,
                    "argmax", color=(255, 0, 0)))
    # 255-valued target pixels: foreground for compute_metrics, dropped with ignore = 255
    t = tgt(52, 3, 24, 40)
    t[0, :, 33:] = 255
    t[1, 20:, :] = 255
    t[2] = 255
    out.append(case("pad255", rnd(54, 3, 2, 24, 40), t, rnd(53, 3, 24, 40, scale=3.0) - 4.0, "argmax", channel=1,
                    color=(10, 200, 255), alpha=0.37, paint=0, ignore=255))
    # K = 4 class ids in the mask; sigmoid of the last channel at 0.3 on the same shape
    out.append(case("k4_argmax", rnd(61, 2, 4, 17, 19), tgt(62, 2, 17, 19, hi=4), rnd(63, 2, 17, 19, scale=1.0),
                    "argmax", alpha=0.5, paint=0))
    out.append(case("k2_sigmoid_ch1", rnd(74, 2, 2, 8, 12), tgt(72, 2, 8, 12), rnd(73, 2, 8, 12, scale=1.0),
                    "sigmoid", channel=1, threshold=0.3, alpha=0.37, color=(0, 0, 255)))
    return out


def write_npz(path, arrays):
    """np.load-compatible archive with fixed member timestamps (np.savez stamps the current time)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    compute_metrics, merge_images = load_reference(args.ref)
    res, names = {}, []
    for c in cases():
        name = c["name"]
        names.append(name)
        inputs = c.get("inputs_of", name)         # cases that share inputs store them once
        res[f"{name}.inputs"] = np.array(inputs)
        if inputs == name:
            for k in ("logits", "target", "frames"):
                res[f"{name}.{k}"] = c[k].numpy()
        res[f"{name}.rule"] = np.array(c["rule"])
        res[f"{name}.channel"] = np.array(c["channel"])
        res[f"{name}.threshold"] = np.array(c["threshold"], dtype=np.float64)
        res[f"{name}.color"] = np.array(c["color"], dtype=np.int64)
        res[f"{name}.alpha"] = np.array(c["alpha"], dtype=np.float64)
        res[f"{name}.paint"] = np.array(c["paint"])
        exp = expected(compute_metrics, merge_images, c)
        for k, v in exp.items():
            res[f"{name}.{k}"] = v
        print(f"{name}: mask sum {int(exp['mask'].sum())}, counts {exp['counts'].tolist()}, "
              f"dice {np.round(exp['dice'], 4).tolist()}")
    res["names"] = np.array(names)
    write_npz(os.path.join(args.out, "predict.npz"), res)


if __name__ == "__main__":
    main()
