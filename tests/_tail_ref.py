"""Case tables, operand builders and float64 references of the head (1-4 classes) and streaming-tail parity tests.

Written from include/stfunet.h and the comments of csrc/head.hip, csrc/stf.hip and csrc/misc.hip, in plain torch
float64 / numpy (on any device), independent of the kernels' loops.  tests/test_tail_parity_cpu.py checks these
references against torch autograd, F.interpolate and F.max_pool2d, that the exact builders keep every sum below
2^24 granules and that the Gaussian seeds leave at most 1e-4 of the mask decisions open;
tests/test_tail_parity_gpu.py runs the tables through the C entry points.

Two operand kinds, as tests/_bn_ref.py.  ``exact``: small integers and dyadic factors, so that every fp32
intermediate is exact in any order, fused or not, and a result EQUALS float64.  ``gauss``: Gaussians rounded to
the storage type; a result stays within a derived bound.  The bound of a sum of n terms, each reached through c
fp32 roundings, is gamma(n + c) * sum |terms| with gamma(m) = m u / (1 - m u), u = 2^-24 (the rigorous form of
(n + c) 2^-24: Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1); a 16-bit output adds half a
storage ulp of the reference.  No constant here is measured on a kernel.
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from _bn_ref import F32, GUARD, SENTINEL, Slice16, half_ulp  # noqa: F401  (the buffers of the BatchNorm parity tests)

U = 2.0 ** -24
f64 = torch.float64
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
EINVAL = 100001
NT = 256                                   # block size of every kernel here
HEAD_TILE_CAP, HEAD_FWD_CAP = 1024, 8192   # csrc/head.hip: backward tiles, forward blocks (4 units a thread a round)


def gamma(m):
    return m * U / (1.0 - m * U)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def ri(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


def un(gen, lo, hi, *shape):
    return (torch.rand(shape, generator=gen) * (hi - lo) + lo).float().double()


def pick(gen, values, *shape):
    return torch.tensor(values, dtype=f64)[torch.randint(0, len(values), shape, generator=gen)]


# ------------------------------------------------------------------ head, 1 to 4 classes
HEAD_K = (1, 2, 3, 4)
HEAD_C = (8, 16, 64, 128, 512)             # C / 8 lanes a pixel: 1 (no lane reduce), 2 (quad), 8 (half row), 16 (row), 64 (cross row)
HEAD_GRID = [(3, 9, 7), (2, 64, 64)]       # the full K x C x storage x BN-state grid runs at these
HEAD_PIXEL = ((1, 1, 1), 3, "fp16")        # (shape, K, storage): one pixel, every C
HEAD_CAP = ((3, 128, 128), 512, 2, "bf16")  # 3.1 M units: past the forward's 8192 blocks x 4, last round partly filled


def head_tiles(P, C):
    return max(1, min(-(-P * (C // 8) // NT), HEAD_TILE_CAP))


class HeadOps:
    """Seeded operands of one head case as float64: y [P][C] (storage-exact), scale, shift, mean, invstd [C],
    w [K][C], bias [K], dl [N][K][H][W]."""

    def __init__(self, shape, C, K, kind, dt, identity):
        N, H, W = shape
        P, ex = N * H * W, kind == "exact"
        g = lambda name, *more: _gen("head", shape, C, kind, name, str(dt) if not ex else "", *more)  # noqa: E731
        self.shape, self.C, self.K, self.kind, self.dt, self.identity = shape, C, K, kind, dt, identity
        self.y = ri(g("y"), -8, 8, P, C) if ex else torch.randn((P, C), generator=g("y")).to(dt).double()
        if identity:                       # nhwc.BNState.identity
            self.scale, self.shift = torch.ones(C, dtype=f64), torch.zeros(C, dtype=f64)
            self.mean, self.invstd = torch.zeros(C, dtype=f64), torch.ones(C, dtype=f64)
        elif ex:
            self.scale = pick(g("scale"), [0.5, 1.0, 2.0], C) * (ri(g("sign"), 0, 1, C) * 2 - 1)
            self.shift = ri(g("shift"), -8, 8, C) / 2
            self.mean = ri(g("mean"), -2, 2, C)
            self.invstd = pick(g("invstd"), [0.5, 1.0, 2.0], C)
        else:
            self.scale = un(g("scale"), 0.5, 1.5, C) * (ri(g("sign"), 0, 1, C) * 2 - 1)
            self.shift, self.mean = un(g("shift"), -0.5, 0.5, C), un(g("mean"), -0.5, 0.5, C)
            self.invstd = un(g("invstd"), 0.5, 2.0, C)
        if ex:
            self.w, self.bias = ri(g("w", K), -4, 4, K, C), ri(g("bias", K), -4, 4, K)
            self.dl = ri(g("dl", K), -3, 3, N, K, H, W)
        else:
            self.w = (torch.randn((K, C), generator=g("w", K)) / 8).float().double()
            self.bias = torch.randn(K, generator=g("bias", K)).float().double()
            self.dl = (torch.randn((N, K, H, W), generator=g("dl", K)) / 16).float().double()

    NAMES = ("y", "scale", "shift", "mean", "invstd", "w", "bias", "dl")

    def to(self, dev):
        for n in self.NAMES:
            setattr(self, n, getattr(self, n).to(dev))
        return self


def head_open(o):
    """Elements whose pre-activation lies within the fp32 slack of zero (two roundings, twice over): the
    kernel's ReLU may fall on either side."""
    z = o.y * o.scale + o.shift
    return z.abs() <= 2.0 ** -22 * ((o.y * o.scale).abs() + o.shift.abs())


def head_ref(o, bounds=True):
    """float64 conv1x1(relu(y*scale + shift)) on the stored y and its backward: logits [N][K][H][W], g [P][C]
    = (dl . w) where z > 0 (UNROUNDED: the kernel stores its rounding and adds the fp32 value into the sums), dW
    [K][C], db [K], sums [2][C] = (sum g, sum g (y - mean) invstd).  With ``bounds``: the any-order fp32 bounds
    b_* of each, ``open`` [P][C] (head_open) and, inside b_sums, the worst case of the open elements."""
    N, K, H, W = o.dl.shape
    P, C = o.y.shape
    z = o.y * o.scale + o.shift
    a = z.clamp_min(0)
    dlp = o.dl.permute(0, 2, 3, 1).reshape(P, K)
    da = dlp @ o.w
    keep = z > 0
    g = torch.where(keep, da, torch.zeros_like(da))
    xh = (o.y - o.mean) * o.invstd
    r = {"logits": (a @ o.w.T + o.bias).view(N, H, W, K).permute(0, 3, 1, 2).contiguous(), "g": g, "dW": dlp.T @ a,
         "db": dlp.sum(0), "sums": torch.stack([g.sum(0), (g * xh).sum(0)])}
    if not bounds:
        return r
    za = (o.y * o.scale).abs() + o.shift.abs()                    # absolute terms of z (z: two roundings)
    daa = dlp.abs() @ o.w.abs()                                    # ... of dl . w (K products, K adds)
    xa = (o.y.abs() + o.mean.abs()) * o.invstd                     # ... of xhat (a difference, a product)
    open_ = z.abs() <= 2.0 ** -22 * za
    zero = torch.zeros_like(daa)
    ga, oa = torch.where(keep, daa, zero), torch.where(open_, daa, zero)
    r["open"] = open_
    # logits: C products of a (2 roundings, relu is 1-Lipschitz) and w, C adds, the bias
    r["b_logits"] = (gamma(C + 4) * (za @ o.w.abs().T + o.bias.abs())).view(N, H, W, K).permute(0, 3, 1, 2)
    r["b_g"] = gamma(K + 1) * daa
    r["b_dW"] = gamma(P + 5) * (dlp.abs().T @ za)                  # P terms dl*a (3 roundings), folds, one fp32 rounding
    r["b_db"] = gamma(P + 2) * dlp.abs().sum(0)
    r["b_sums"] = torch.stack([gamma(P + K + 2) * ga.sum(0) + oa.sum(0),
                               gamma(P + K + 5) * (ga * xa).sum(0) + (oa * xa).sum(0)])
    return r


def head_granules(o):
    """Largest sum of absolute terms behind any output of the exact run, in units of its granule (0.5: scale,
    shift / 2 and invstd are multiples of 0.5, everything else an integer).  Below 2^24 every partial sum, in any
    order and any tiling, is an integer number of granules that fp32 holds."""
    P, K = o.y.shape[0], o.w.shape[0]
    za = (o.y * o.scale).abs() + o.shift.abs()
    dlp = o.dl.permute(0, 2, 3, 1).reshape(P, K).abs()
    daa = dlp @ o.w.abs()
    ga = torch.where(o.y * o.scale + o.shift > 0, daa, torch.zeros_like(daa))
    xa = (o.y.abs() + o.mean.abs()) * o.invstd
    return {"logits": float((za @ o.w.abs().T + o.bias.abs()).max() / 0.5), "g": float(daa.max()),
            "dW": float((dlp.T @ za).max() / 0.5), "db": float(dlp.sum(0).max()),
            "sum_g": float(ga.sum(0).max()), "sum_gx": float((ga * xa).sum(0).max() / 0.5)}


# ------------------------------------------------------------------ MaxPool(3, 2, 1)
POOL_HW = [(1, 1), (1, 5), (2, 3), (7, 7), (15, 16)]
POOL_C = (8, 64)
POOL_N = 2


def pool_input(H, W, C):
    """[N][C][H][W] small integers: many ties; channel 1 mod 4 all negative, channel 2 mod 4 constant."""
    x = ri(_gen("pool", H, W, C), -2, 2, POOL_N, C, H, W)
    x[:, 1::4] -= 3
    x[:, 2::4] = -1
    return x


def pool_out(n):
    return (n - 1) // 2 + 1


def pool_codes(idx, H, W):
    """F.max_pool2d's flat input index [N][C][Ho][Wo] -> the window position dy*3 + dx the kernel records."""
    Ho, Wo = idx.shape[-2:]
    oy = torch.arange(Ho).view(Ho, 1)
    ox = torch.arange(Wo).view(1, Wo)
    return ((idx // W - (2 * oy - 1)) * 3 + (idx % W - (2 * ox - 1))).to(torch.uint8)


def pool_ref(x, dout=None):
    """F.max_pool2d(3, 2, 1) of x [N][C][H][W] float64: (out, codes) and, with dout, its float64 backward and the
    sum of the absolute terms of every input element."""
    H, W = x.shape[-2:]
    xr = x.clone().requires_grad_(True)
    out, idx = F.max_pool2d(xr, 3, 2, 1, return_indices=True)
    if dout is None:
        return out.detach(), pool_codes(idx, H, W)
    dx, = torch.autograd.grad(out, xr, dout)
    flat = torch.zeros(x.shape[0], x.shape[1], H * W, dtype=f64)
    flat.scatter_add_(2, idx.flatten(2), dout.abs().flatten(2))
    return out.detach(), pool_codes(idx, H, W), dx, flat.view_as(x)


def nhwc(x):
    """[N][C][H][W] -> [N*H*W][C]"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def nchw(m, N, H, W):
    """[N*H*W][C] -> [N][C][H][W]"""
    return m.view(N, H, W, -1).permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------ bilinear, align_corners=True
# (H, W, h, w): the input is H x W, the output h x w
RESIZE = [(64, 48, 3, 2), (3, 2, 64, 48), (33, 17, 17, 9), (17, 9, 33, 17), (2, 2, 2, 2), (1, 4, 3, 1), (7, 9, 13, 17)]
RESIZE_DYADIC = {(33, 17, 17, 9), (17, 9, 33, 17), (2, 2, 2, 2)}       # every lambda is 0 or 0.5: the exact run
RESIZE_C = (8, 64)
RESIZE_N = 2


def ac_table(n_in, n_out):
    """PyTorch's fp32 coordinate arithmetic (upsample_bilinear2d, align_corners=True) in numpy float32:
    i0, i1 (int), lambda0 = 1 - lambda1 and lambda1 (float32)."""
    sc = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    f = (sc * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = np.minimum(f.astype(np.int32), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (f - i0.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1) - l1).astype(np.float32)
    return i0, i1, l0, l1


def ac_matrix(n_in, n_out):
    """The table as a float64 matrix [n_out][n_in] and, per input index, how many outputs read it."""
    i0, i1, l0, l1 = ac_table(n_in, n_out)
    A = np.zeros((n_out, n_in))
    o = np.arange(n_out)
    np.add.at(A, (o, i0), l0.astype(np.float64))
    np.add.at(A, (o, i1), l1.astype(np.float64))
    return torch.from_numpy(A), torch.from_numpy((A != 0).sum(0))


def resize_fwd(x, h, w):
    """x [N][H][W][C] float64 -> (y [N][h][w][C], the sum of the absolute terms).  Four terms, each through two
    products and two adds: gamma(7) of the absolute terms."""
    Ay, Ax = ac_matrix(x.shape[1], h)[0].to(x.device), ac_matrix(x.shape[2], w)[0].to(x.device)
    e = lambda a, b, t: torch.einsum("ab,nbdc,ed->naec", a, t, b)  # noqa: E731
    return e(Ay, Ax, x), e(Ay.abs(), Ax.abs(), x.abs())


def resize_bwd(dy, H, W):
    """The adjoint scattered from the same tables: dy [N][h][w][C] -> (dx [N][H][W][C], the absolute terms, the
    number of terms of every input pixel [H][W])."""
    (Ay, cy), (Ax, cx) = ac_matrix(H, dy.shape[1]), ac_matrix(W, dy.shape[2])
    Ay, Ax = Ay.to(dy.device), Ax.to(dy.device)
    e = lambda a, b, t: torch.einsum("ab,naec,ed->nbdc", a, t, b)  # noqa: E731
    return e(Ay, Ax, dy), e(Ay.abs(), Ax.abs(), dy.abs()), (cy.view(H, 1) * cx.view(1, W)).to(dy.device)


def resize_input(shape, kind, dt, name, *dims):
    """Multiples of 1/4 in [-2, 2] (exact) or Gaussians rounded to ``dt`` (None: fp32), as float64."""
    g = _gen("resize", shape, kind, name, str(dt) if kind == "gauss" else "", dims)
    if kind == "exact":
        return ri(g, -8, 8, *dims) / 4
    v = torch.randn(dims, generator=g)
    return (v if dt is None else v.to(dt)).double()


# ------------------------------------------------------------------ pack_input / pack_sequence
PACK_C = [(1, 8), (3, 8), (8, 8), (9, 16)]            # (C, Cpad)


def pack_values(dt, n, seed):
    """n fp32 values whose rounding to ``dt`` is decided at the last bit: midpoints of neighbouring 16-bit
    values and their fp32 neighbours, 16-bit subnormals and the ties below them, +-0, +-inf, NaN, values that
    overflow ``dt``, and Gaussians."""
    gen = _gen("pack", str(dt), seed)
    base = (torch.randn(96, generator=gen) * 4).to(dt)
    nxt = (base.view(torch.int16) + 1).view(dt)                     # next magnitude
    mid = (base.float() + nxt.float()) / 2                          # exact in fp32: a tie
    inf = torch.tensor(float("inf"))
    tiny = 2.0 ** -24 if dt is torch.float16 else 2.0 ** -133       # the smallest 16-bit subnormal
    sub = torch.tensor([tiny * k / 2 for k in range(1, 12)], dtype=torch.float64).float()
    big = torch.tensor([65504.0, 65519.99, 65520.0, 65536.0, 1e5, 3.3e38, 3.4028234e38] if dt is torch.float16
                       else [3.3895314e38, 3.3961775e38, 3.4e38, 3.4028234e38, 65520.0, 1e5, 2.0 ** 127])
    sp = torch.cat([mid, torch.nextafter(mid, inf), torch.nextafter(mid, -inf), sub, torch.nextafter(sub, inf),
                    big, torch.tensor([0.0, float("inf"), float("nan"), 1.0, 2.0 ** -126, 2.0 ** -149])])
    sp = torch.cat([sp, -sp])
    pool = torch.cat([sp, torch.randn(max(n - sp.numel(), 0), generator=gen)])      # n < the specials: a subset
    return pool[torch.randperm(pool.numel(), generator=gen)][:n].float()


def pack_input_ref(x, cpad, dt):
    """x [N][C][H][W] fp32 -> [N*H*W][cpad] of ``dt``: torch's round to nearest even, zero padding."""
    N, C, H, W = x.shape
    out = torch.zeros(N * H * W, cpad, dtype=dt)
    out[:, :C] = nhwc(x).to(dt)
    return out


def pack_sequence_ref(x, T, P, cpad, dt):
    """x [B][Ttot][C][H][W] fp32 -> [(t*B + b)*H*W][cpad]: frame t's C channels, then channel 0 of the frames
    T .. T+P-1, then zeros."""
    B, _, C, H, W = x.shape
    out = torch.zeros(T, B, H, W, cpad, dtype=dt)
    out[..., :C] = x[:, :T].permute(1, 0, 3, 4, 2).to(dt)
    for p in range(P):
        out[..., C + p] = x[:, T + p, 0].to(dt).unsqueeze(0)
    return out.view(-1, cpad)


def same16(got, want):
    """Bit-equal 16-bit tensors, NaN matching any NaN."""
    gn, wn = torch.isnan(got), torch.isnan(want)
    return bool((gn == wn).all()) and bool((got.view(torch.int16) == want.view(torch.int16))[~wn].all())


# ------------------------------------------------------------------ channel_sum / stat_sums
CSUM_C = (8, 64, 512)
CSUM_M = (1, 257, 70000)                   # 70 000 x 64 / 8 units: past the 1024-tile cap, second grid-stride pass
FOLD_LANES = 64                            # row-lanes of a 1024-thread fold16 block; its unrolled round takes 4 x 64 rows
STAT_TILES = (1, 63, 64, 65, 255, 256, 257, 700)
STAT_COLS = [(40, 8, 24), (16, 0, 16), (13, 3, 5), (64, 31, 33)]     # (Nout, c0, C)


def csum_tiles(M, C):
    return max(1, min(-(-M * (C // 8) // NT), 1024))
