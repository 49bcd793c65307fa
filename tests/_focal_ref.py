"""Vectorised torch restatement of the criterion with a focal cross-entropy and a Tversky overlap
(tests only).

The reference project has neither term, so no fixture pins this file; test_focal_tversky_cpu.py pins it
to ``_criterion_ref.criterion_ref`` at gamma = 0, alpha = beta = 1/2 and to the closed-form gradient below.
For softmax p, target t, mask m = (t != ignore_index) when ignore_index >= 0 (else all ones), class
weights w (ones when absent), q = p_t, nll = -log q, N images, K classes:

    CE_f = sum m w[t] (1-q)^gamma nll / sum m w[t]                    (gamma = 0: the cross-entropy)
    I    = sum_pixels m p_k [t = k],  P = sum m p_k,  T = sum m [t = k]      per (image, class)
    D    = (2 I + eps) / (2 I + 2 alpha (P - I) + 2 beta (T - I) + eps), and 1 where P + T == 0
    loss = CE_f + (1 - mean_k mean_b D  if dice else 0)

1-q is the sum of the other classes' probabilities (never ``1 - q``: in float64 that is exactly 0 from
logit gaps of about 37 on, and the power's derivative there is not finite); where it is exactly 0
(K = 1) and gamma > 0 the factor is the constant 0.  Runs in the dtype of ``logits`` (the tests pass
float64 on the CPU); gradients by autograd.
"""
import torch


def _parts(logits, target, weight, ignore_index):
    N, K = logits.shape[:2]
    z = logits.reshape(N, K, -1)
    t = target.reshape(N, -1).long()
    m = (t != ignore_index) if ignore_index >= 0 else torch.ones_like(t, dtype=torch.bool)
    tc = torch.where(m, t, torch.zeros_like(t))
    w = torch.ones(K, dtype=z.dtype) if weight is None else torch.as_tensor(weight).to(z.dtype)
    wt = w[tc] * m
    mk = m[:, None].to(z.dtype)
    oh = torch.nn.functional.one_hot(tc, K).permute(0, 2, 1).to(z.dtype)
    return z, wt, mk, oh


def focal_tversky_ref(logits, target, weight=None, ignore_index=-100, dice=True, gamma=0.0, alpha=0.5, beta=0.5,
                      eps=1e-6):
    z, wt, mk, oh = _parts(logits, target, weight, ignore_index)
    p = torch.softmax(z, 1)
    nll = -(torch.log_softmax(z, 1) * oh).sum(1)
    if gamma == 0:
        f = torch.ones_like(nll)
    else:
        om = (p * (1 - oh)).sum(1)                       # 1 - q
        pos = om > 0
        f = torch.where(pos, torch.where(pos, om, torch.ones_like(om)) ** gamma, torch.zeros_like(om))
    loss = (wt * f * nll).sum() / wt.sum()
    if dice:
        pm, tm = p * mk, oh * mk
        inter, ps, ts = (pm * tm).sum(-1), pm.sum(-1), tm.sum(-1)
        d = (2 * inter + eps) / (2 * inter + 2 * alpha * (ps - inter) + 2 * beta * (ts - inter) + eps)
        d = torch.where(ps + ts == 0, torch.ones_like(d), d)
        loss = loss + 1 - d.mean()
    return loss


def ref_loss_and_grad(logits, target, weight=None, ignore_index=-100, dice=True, gamma=0.0, alpha=0.5, beta=0.5,
                      grad_out=1.0):
    """float64 CPU loss (python float) and d(grad_out * loss)/d(logits) of ``focal_tversky_ref``."""
    x = logits.detach().double().cpu().requires_grad_(True)
    w = None if weight is None else torch.as_tensor(weight).double().cpu()
    loss = focal_tversky_ref(x, target.detach().cpu(), w, ignore_index, dice, gamma, alpha, beta)
    (loss * grad_out).backward()
    return loss.item(), x.grad


def closed_form_grad(logits, target, weight=None, ignore_index=-100, dice=True, gamma=0.0, alpha=0.5, beta=0.5,
                     eps=1e-6):
    """The backward the kernels implement, written out (no autograd), in the dtype of ``logits``:
    dz_k = m c w[t] (p_k - t_k)/Wsum + m p_k (G_k - sum_j p_j G_j),
    c = (1-q)^(gamma-1) ((1-q) + gamma q nll) (1 at gamma = 0, 0 where 1-q == 0 and gamma > 0),
    G_k = -(1/(K N)) (2 t_k/den - (2I+eps) (2(1-alpha-beta) t_k + 2 alpha)/den^2),
    den = 2(1-alpha-beta) I + 2 alpha P + 2 beta T + eps; G = 0 with Dice off or where P + T == 0."""
    N, K = logits.shape[:2]
    z, wt, mk, oh = _parts(logits.detach(), target, weight, ignore_index)
    p = torch.softmax(z, 1)
    q = (p * oh).sum(1)
    nll = -(torch.log_softmax(z, 1) * oh).sum(1)
    om = (p * (1 - oh)).sum(1)
    if gamma == 0:
        c = torch.ones_like(om)
    else:
        pos = om > 0
        c = torch.where(pos, torch.where(pos, om, torch.ones_like(om)) ** (gamma - 1) * (om + gamma * q * nll),
                        torch.zeros_like(om))
    g = (wt * c / wt.sum())[:, None] * (p - oh)
    if dice:
        pm, tm = p * mk, oh * mk
        inter, ps, ts = (pm * tm).sum(-1), pm.sum(-1), tm.sum(-1)
        rest = 2 * (1 - alpha - beta)
        den = rest * inter + 2 * alpha * ps + 2 * beta * ts + eps
        num = (2 * inter + eps) / den ** 2
        live = (ps + ts != 0).to(z.dtype)
        ga = -(2 / den - num * rest) * live / (K * N)
        gb = num * 2 * alpha * live / (K * N)
        G = ga[..., None] * oh + gb[..., None]
        g = g + pm * (G - (p * G).sum(1, keepdim=True))
    return (g * mk).reshape(logits.shape)
