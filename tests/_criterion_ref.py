"""Vectorised torch restatement of the criterion with its options (tests only).

For softmax p, target t, mask m = (t != ignore_index) when ignore_index >= 0 (else all
ones), class weights w (ones when absent), N images, K classes:

    CE   = sum m w[t] (-log p_t) / sum m w[t]
    I    = sum_pixels m p_k [t = k],  S = sum m p_k + sum m [t = k]     per (image, class)
    D    = (2 I + eps) / (S + eps), and 1 where S == 0 (an image with every pixel ignored)
    loss = CE + (1 - mean_k mean_b D  if dice else 0)

Runs in the dtype of ``logits`` (the tests pass float64 on the CPU); gradients by autograd.
"""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def criterion_ref(logits, target, weight=None, ignore_index=-100, dice=True, eps=1e-6):
    N, K = logits.shape[:2]
    z = logits.reshape(N, K, -1)
    t = target.reshape(N, -1).long()
    m = (t != ignore_index) if ignore_index >= 0 else torch.ones_like(t, dtype=torch.bool)
    tc = torch.where(m, t, torch.zeros_like(t))
    w = torch.ones(K, dtype=z.dtype) if weight is None else torch.as_tensor(weight).to(z.dtype)
    wt = w[tc] * m
    nll = -torch.log_softmax(z, 1).gather(1, tc[:, None]).squeeze(1)
    loss = (wt * nll).sum() / wt.sum()
    if dice:
        mk = m[:, None].to(z.dtype)
        p = torch.softmax(z, 1) * mk
        oh = torch.nn.functional.one_hot(tc, K).permute(0, 2, 1).to(z.dtype) * mk
        inter = (p * oh).sum(-1)
        sets = p.sum(-1) + oh.sum(-1)
        d = torch.where(sets == 0, torch.ones_like(sets), (2 * inter + eps) / (sets + eps))
        loss = loss + 1 - d.mean()
    return loss


def ref_loss_and_grad(logits, target, weight=None, ignore_index=-100, dice=True, grad_out=1.0):
    """float64 CPU loss (python float) and d(grad_out * loss)/d(logits) of ``criterion_ref``."""
    x = logits.detach().double().cpu().requires_grad_(True)
    w = None if weight is None else torch.as_tensor(weight).double().cpu()
    loss = criterion_ref(x, target.detach().cpu(), w, ignore_index, dice)
    (loss * grad_out).backward()
    return loss.item(), x.grad


def fixture_entries():
    """The reference-generated cases of tests/golden/criterion_options.npz as dicts."""
    g = np.load(os.path.join(GOLDEN, "criterion_options.npz"))
    out = []
    for name in g["names"].tolist():
        w = g[name + ".weight"]
        case = str(g[name + ".case"])
        out.append(dict(name=name, logits=torch.from_numpy(g[case + ".logits"]),
                        target=torch.from_numpy(g[case + ".target"]),
                        weight=torch.from_numpy(w) if w.size else None,
                        ignore_index=int(g[name + ".ignore_index"]), dice=bool(g[name + ".dice"]),
                        loss=float(g[name + ".loss"]), grad=torch.from_numpy(g[name + ".grad"])))
    return out


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()
