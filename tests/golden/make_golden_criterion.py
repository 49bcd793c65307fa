"""Generate tests/golden/criterion_options.npz by running the REFERENCE criterion.

    python tests/golden/make_golden_criterion.py  [--ref /root/reference]

``criterion(inputs, target, loss_weight, num_classes, dice, ignore_index)``
(train_utils/train_and_eval.py:299-313, imported by path through make_golden.load_reference)
on N = 3 images of 8 x 12 pixels, for K in {2, 3} x class weights {absent, present} x Dice
{on, off} x ignore_index {-100, 255}.  With 255, image 0 is ignored in a column band, image 1
in a row band and image 2 everywhere (its Dice is the empty-set 1).  Each entry ``<name>.*``
holds weight (empty = None), ignore_index, dice, the loss and its autograd gradient, and
``<name>.case`` names the ``<case>.logits`` / ``<case>.target`` it ran on (shared by the four
entries of one K and ignore_index); ``names`` lists the entries.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import load_reference  # noqa: E402

N, H, W = 3, 8, 12
WEIGHTS = {2: [0.3, 1.7], 3: [0.25, 1.5, 2.0]}


def case(K, ignore_index, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(N, K, H, W, generator=g) * 2.0
    target = torch.randint(0, K, (N, H, W), generator=g)
    if ignore_index >= 0:
        target[0, :, 9:] = ignore_index
        target[1, 6:, :] = ignore_index
        target[2] = ignore_index
    return logits, target


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    tae = load_reference(args.ref)[2]
    res, names = {}, []
    for K in (2, 3):
        for ign in (-100, 255):
            logits, target = case(K, ign, seed=100 * K + (ign > 0))
            cname = f"k{K}_i{ign if ign > 0 else 'none'}"
            res[cname + ".logits"] = logits.numpy()
            res[cname + ".target"] = target.numpy()
            for weighted in (0, 1):
                for dice in (1, 0):
                    name = f"{cname}_w{weighted}_d{dice}"
                    w = torch.tensor(WEIGHTS[K]) if weighted else None
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
    np.savez_compressed(os.path.join(args.out, "criterion_options.npz"), **res)


if __name__ == "__main__":
    main()
