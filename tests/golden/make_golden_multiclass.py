"""Generate tests/golden/multiclass.npz and multiclass_keys.json by running the REFERENCE.

    python tests/golden/make_golden_multiclass.py  [--ref /root/reference]

``criterion(inputs, target, loss_weight, num_classes, dice, ignore_index)``
(train_utils/train_and_eval.py:299-313, imported by path through make_golden.load_reference)
with ``loss.backward()`` on N = 3 images of 7 x 9 pixels, logits ``randn * 2``, for K in
{5, 7, 16} x class weights {absent, present} x Dice {on, off} x ignore_index {-100, 255}.  With
255, image 0 is ignored in a column band, image 1 in a row band and image 2 everywhere (its Dice
is the empty-set 1), as in make_golden_criterion.py.  The entry layout is that script's
(``<name>.weight`` / ``.ignore_index`` / ``.dice`` / ``.loss`` / ``.grad`` / ``.case``, ``names``).

multiclass_keys.json: state_dict key order and shapes, and the parameter count, of the
reference ``UNet(in_channels=8, num_classes=6, base_c=8)`` (src/unet.py).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import load_reference  # noqa: E402

N, H, W = 3, 7, 9
CLASSES = (5, 7, 16)


def weights(K):
    return [0.25 + 0.35 * ((3 * k) % K) for k in range(K)]


def case(K, ignore_index, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(N, K, H, W, generator=g) * 2.0
    target = torch.randint(0, K, (N, H, W), generator=g)
    if ignore_index >= 0:
        target[0, :, 6:] = ignore_index
        target[1, 5:, :] = ignore_index
        target[2] = ignore_index
    return logits, target


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    unet_mod, _, tae, _ = load_reference(args.ref)
    res, names = {}, []
    for K in CLASSES:
        for ign in (-100, 255):
            logits, target = case(K, ign, seed=100 * K + (ign > 0))
            cname = f"k{K}_i{ign if ign > 0 else 'none'}"
            res[cname + ".logits"] = logits.numpy()
            res[cname + ".target"] = target.numpy()
            for weighted in (0, 1):
                for dice in (1, 0):
                    name = f"{cname}_w{weighted}_d{dice}"
                    w = torch.tensor(weights(K)) if weighted else None
                    x = logits.clone().requires_grad_(True)
                    loss = tae.criterion({"out": x}, target, loss_weight=w, num_classes=K, dice=bool(dice),
                                         ignore_index=ign)
                    loss.backward()
                    names.append(name)
                    res[name + ".case"] = np.array(cname)
                    res[name + ".weight"] = (w if weighted else torch.zeros(0)).numpy()
                    res[name + ".ignore_index"] = np.array(ign)
                    res[name + ".dice"] = np.array(dice)
                    res[name + ".loss"] = np.array(loss.item(), dtype=np.float64)
                    res[name + ".grad"] = x.grad.numpy()
                    print(f"{name}: loss {loss.item():.6f}")
    res["names"] = np.array(names)
    np.savez_compressed(os.path.join(args.out, "multiclass.npz"), **res)
    m = unet_mod.UNet(in_channels=8, num_classes=6, base_c=8)
    keys = {"unet_in8_k6_c8": [[n, list(v.shape)] for n, v in m.state_dict().items()],
            "param_count": sum(p.numel() for p in m.parameters())}
    with open(os.path.join(args.out, "multiclass_keys.json"), "w") as f:
        json.dump(keys, f)


if __name__ == "__main__":
    main()
