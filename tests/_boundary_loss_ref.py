"""Reference restatement of the boundary loss (Kervadec et al., MIDL 2019) for the tests.

The signed distance maps with ``scipy.ndimage.distance_transform_edt`` and the project's empty / full
rule, the term in float64 torch (gradients by autograd), the closed-form gradient of INTEGRATION.md
2.1 written out, and the sum of the absolute terms that the loss tolerance scales with.  Also the
target contents the map tests share.
"""
import numpy as np
import torch
from scipy.ndimage import distance_transform_edt


def sdf_ref(target, K, ignore_index=None):
    """np.float32 [N, K-1, H, W]: channel k-1 for class k with G = {target == k} (never the ignore
    value): +d(q, G) outside G, 1 - d(q, not G) inside, 0 everywhere where G is empty or full."""
    t = np.asarray(target)
    N, H, W = t.shape
    out = np.zeros((N, K - 1, H, W), np.float32)
    for n in range(N):
        for k in range(1, K):
            G = t[n] == k
            if ignore_index is not None and ignore_index >= 0:
                G &= t[n] != ignore_index
            if not G.any() or G.all():
                continue
            outside = distance_transform_edt(~G)          # distance to the nearest pixel of G
            inside = distance_transform_edt(G)            # distance to the nearest pixel outside G
            out[n, k - 1] = np.where(G, 1.0 - inside, outside).astype(np.float32)
    return out


def sdf_brute(target, K, ignore_index=None):
    """The same from the O(n^2) integer squared distance: float32(sqrt(float64(d2)))."""
    t = np.asarray(target)
    N, H, W = t.shape
    ys, xs = np.mgrid[0:H, 0:W]
    out = np.zeros((N, K - 1, H, W), np.float32)
    for n in range(N):
        for k in range(1, K):
            G = t[n] == k
            if ignore_index is not None and ignore_index >= 0:
                G &= t[n] != ignore_index
            if not G.any() or G.all():
                continue
            for y in range(H):
                for x in range(W):
                    other = ~G if G[y, x] else G
                    d2 = int((((ys - y) ** 2 + (xs - x) ** 2)[other]).min())
                    d = np.sqrt(np.float64(d2))
                    out[n, k - 1, y, x] = np.float32(1.0 - d) if G[y, x] else np.float32(d)
    return out


def _mask(target, ignore_index):
    if ignore_index is not None and ignore_index >= 0:
        return (target != ignore_index).to(torch.float64)
    return torch.ones(target.shape, dtype=torch.float64)


def boundary_loss_ref(logits, target, phi, ignore_index=-100):
    """(loss, grad) in float64: L_B = sum m p_k phi_k / ((K-1) M) over k >= 1, the gradient by autograd."""
    x = logits.detach().to(torch.float64).requires_grad_(True)
    K = x.shape[1]
    p = torch.softmax(x, dim=1)
    m = _mask(target, ignore_index)
    f = torch.as_tensor(phi).to(torch.float64)
    loss = (m[:, None] * p[:, 1:] * f).sum() / ((K - 1) * m.sum())
    loss.backward()
    return loss.item(), x.grad


def closed_form_grad(logits, target, phi, ignore_index=-100):
    """dz_j = m p_j (phi_j - sum_{c >= 1} p_c phi_c) / ((K-1) M) with phi_0 = 0, float64."""
    x = logits.detach().to(torch.float64)
    N, K, H, W = x.shape
    p = torch.softmax(x, dim=1)
    m = _mask(target, ignore_index)
    f = torch.cat([torch.zeros(N, 1, H, W, dtype=torch.float64), torch.as_tensor(phi).to(torch.float64)], dim=1)
    a = (p * f).sum(dim=1, keepdim=True)
    return m[:, None] * p * (f - a) / ((K - 1) * m.sum())


def abs_loss(logits, target, phi, ignore_index=-100):
    """sum m p_k |phi_k| / ((K-1) M): what an fp32 sum's error scales with."""
    x = logits.detach().to(torch.float64)
    K = x.shape[1]
    p = torch.softmax(x, dim=1)
    m = _mask(target, ignore_index)
    f = torch.as_tensor(phi).to(torch.float64).abs()
    return ((m[:, None] * p[:, 1:] * f).sum() / ((K - 1) * m.sum())).item()


# ---------------------------------------------------------------- target contents of the map tests
def blobs(N, K, H, W, density, seed):
    """Class k >= 1 at about ``density`` of the pixels in total, class 0 elsewhere."""
    g = torch.Generator().manual_seed(seed)
    fg = torch.rand(N, H, W, generator=g) < density
    return torch.where(fg, torch.randint(1, K, (N, H, W), generator=g), torch.zeros(N, H, W, dtype=torch.long))


def one_pixel(N, K, H, W, corner=False):
    t = torch.zeros(N, H, W, dtype=torch.long)
    for n in range(N):
        y, x = (H - 1, W - 1) if corner else ((n + H // 2) % H, (2 * n + W // 3) % W)
        t[n, y, x] = 1 + n % (K - 1)
    return t


def checkerboard(N, K, H, W):
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    t = ((ys + xs) % 2) * (1 + (ys + 2 * xs) % (K - 1))
    return t[None].repeat(N, 1, 1).long()


def absent_and_full(N, K, H, W, seed):
    """Random classes, but class 1 is absent from image 0 and fills the last image."""
    t = blobs(N, K, H, W, 0.5, seed)
    t[0][t[0] == 1] = 0
    t[-1] = 1
    return t


def empty_rows(N, K, H, W, seed):
    """Sites only in every third row (and none of class 0 there in odd images): rows without a site of
    either side lie between rows that have some."""
    t = torch.zeros(N, H, W, dtype=torch.long)
    b = blobs(N, K, H, W, 0.3, seed)
    t[:, ::3] = b[:, ::3]
    if N > 1:
        t[1::2, 1::3] = 1                   # whole rows of class 1: no site of "not G" in those rows
    return t


def padded(N, K, H, W, seed):
    """255 on the right and at the bottom, as ``collate_fn`` pads a mixed-size batch."""
    t = blobs(N, K, H, W, 0.5, seed)
    t[:, :, W - max(1, W // 4):] = 255
    t[:, H - max(1, H // 4):, :] = 255
    return t
