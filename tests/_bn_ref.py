"""Case table, operand builders and float64 reference of the BatchNorm parity tests.

Written from include/stfunet.h and the comment at the top of csrc/bn.hip, in plain torch float64 (on
any device), independent of the kernels and of tests/_bn_bits.py.  tests/test_bn_parity_cpu.py checks
this reference against torch autograd and that every case of the table has the edge it is listed for;
tests/test_bn_parity_gpu.py runs the table through the C entry points.

Layout: a 16-bit tensor is [M][C] (M = N*H*W pixels, NHWC), a per-group vector [G][C]; group g owns the
pixels [g*Mg, (g+1)*Mg).  Shapes are (N, H, W, C, groups).

Two operand kinds.  ``exact``: dyadic values -- 16-bit tensors multiples of 0.25 in [-2, 2]; scale, rscale
in {+-0.5, +-1, +-2}; invstd in {0.5, 1, 2}; shift, mean multiples of 1/4 in [-1, 1]; rshift, coef
multiples of 1/8 -- so y*scale + shift is a multiple of 1/8 below 32 (exact in bf16 and fp16, and a
visible share is exactly 0), every product and every sum is exact in fp32 in any order, fused or not, as
long as a sum stays below 2^24 granules (``granules``; the CPU test asserts it), and windows hold ties.
``gauss``: Gaussians rounded to the storage type, fp32 vectors uniform.
"""
import zlib

import numpy as np
import torch

NT, UPT, PNT, ROW_CAP, RUN_BATCH = 256, 4, 512, 1024, 32      # csrc/bn.hip's constants
ACT_CAP = 8192                          # block cap of stf_bn_act and of stf_bn_bwd_apply without bias sums
PAD, OFF = 16, 8                        # wide buffers: C + PAD channels, the slice starts at OFF
GUARD = 1024                            # sentinel floats each side of an fp32 buffer
SENTINEL = 0x7FC0BEEF                   # their bits: a NaN that nothing computes
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
MOM, EPS = float(np.float32(0.1)), float(np.float32(1e-5))
U23 = 2.0 ** -23
EINVAL = 100001

# ------------------------------------------------------------------ the table
# group-major act / reduce / apply: (shape, edge)
GROUP_MAJOR = [
    ((2, 3, 3, 8, 1), "below_block"),             # 18 units: part of one 256-thread chunk
    ((4, 9, 15, 64, 2), "ragged_idle"),           # 3 blocks per group, the last ends in its first chunk; idle reduce blocks
    ((1, 3, 3, 2048, 1), "ragged_idle"),          # C / 8 = 256: one thread per chunk of a pixel
    ((128, 33, 32, 64, 128), "second_iter"),      # capped reduce / bias grid: second grid-stride iteration, ragged
    ((128, 91, 91, 8, 128), "second_iter"),       # ... with one chunk per pixel.  dbias: see DBIAS_BOUNDED
]
# dbias of this shape sums 1.06 M terms of up to 160 granules: past 2^24, so the exact run compares it
# under the bounded run's rule (every other output of the case stays exact)
DBIAS_BOUNDED = {(128, 91, 91, 8, 128)}
BIG = (2, 725, 724, 64, 1)                        # 8.4 M units: past the 8192-block cap of act and plain apply
GENERIC = [(2, 3, 5, 24, 1), (4, 3, 5, 24, 2), (3, 2, 3, 4096, 3)]      # C / 8 divides no block
POOL_ACT = [(4, 6, 10, 8, 2), (4, 6, 10, 64, 2), (2, 6, 10, 1024, 2)]
POOL_DPP = [((4, 6, 10, 8, 2), "dpp"), ((4, 6, 10, 64, 2), "dpp"), ((2, 6, 10, 512, 2), "dpp"),
            ((128, 34, 32, 64, 128), "dpp_unpaired")]
POOL_WIN = [((2, 6, 10, 1024, 2), "win"), ((2, 4, 6, 2048, 1), "win")]
POOL3 = [((2, 9, 11, 64, 2), "pool3"), ((2, 8, 8, 64, 1), "pool3"), ((2, 1, 5, 8, 1), "pool3"),
         ((2, 2, 1, 8, 2), "pool3"), ((1, 5, 2, 2048, 1), "pool3"), ((128, 46, 46, 64, 128), "pool3_second")]
# finalize / bwd_finalize: (tiles, C, groups)
FINALIZE = [(1, 8, 1), (37, 24, 3), (37, 2048, 3), (1024, 64, 3), (1024, 2048, 1), (1025, 64, 1), (1025, 24, 3),
            (5000, 8, 3), (5000, 2048, 1)]
BATCH_COUNTS = (33, 70)


def cg_ok(C):
    return C >= 8 and C % 8 == 0 and NT % (C // 8) == 0


def g_tiles(upg, groups, cap):
    """Blocks per group of the group-major kernels, from the file's constants."""
    return max(1, min(-(-upg // (NT * UPT)), max(cap // groups, 1)))


def reduce_tiles(upg, groups):
    return max(1, min(-(-upg // NT), -(-ROW_CAP // groups)))


# ------------------------------------------------------------------ operands
class Ops:
    """The seeded operands of one (shape, kind, storage type), made on the CPU when first asked for, as
    float64 on ``dev``.  ``dev_gen``: draw on the device (the 67 M-element case)."""

    def __init__(self, shape, kind, dt, dev="cpu", dev_gen=False):
        self.shape, self.kind, self.dt, self.dev, self.t = shape, kind, dt, dev, {}
        self.gdev = dev if dev_gen else "cpu"

    def __getitem__(self, name):
        if name not in self.t:
            seed = zlib.crc32(repr((self.shape, self.kind, name, str(self.dt) if self.kind == "gauss" else "")).encode())
            gen = torch.Generator(device=self.gdev).manual_seed(seed)
            self.t[name] = self._make(name, gen).to(self.dev)
        return self.t[name]

    def _make(self, name, gen):
        N, H, W, C, G = self.shape
        M, exact, d = N * H * W, self.kind == "exact", self.gdev
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen, device=d).double()  # noqa: E731
        un = lambda lo, hi, *s: (torch.rand(s, generator=gen, device=d) * (hi - lo) + lo).float().double()  # noqa: E731
        if name in ("y", "dz", "res", "g", "msrc", "dpool", "dout"):
            rows = {"dpool": M // 4, "dout": N * Ho * Wo}.get(name, M)
            if exact:
                return ri(0 if name == "msrc" else -8, 8, rows, C) / 4
            return torch.randn((rows, C), generator=gen, device=d).to(self.dt).double()
        if name == "argmax_rand":
            return torch.randint(0, 9, (N * Ho * Wo, C), generator=gen, device=d, dtype=torch.uint8)
        if name in ("scale", "rscale"):
            if exact:
                return torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64, device=d)[ri(0, 2, G, C).long()] * \
                    (ri(0, 1, G, C) * 2 - 1)
            return un(0.5, 1.5, G, C) * (ri(0, 1, G, C) * 2 - 1)
        if name == "invstd":
            if exact:
                return torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64, device=d)[ri(0, 2, G, C).long()]
            return un(0.5, 2.0, G, C)
        if name in ("shift", "mean"):
            return ri(-4, 4, G, C) / 4 if exact else un(-0.5, 0.5, G, C)
        if name == "rshift":
            return ri(-4, 4, G, C) / 8 if exact else un(-0.5, 0.5, G, C)
        if name == "coef":
            return ri(-8, 8, G, 3, C) / 8 if exact else un(-1.0, 1.0, G, 3, C)
        raise KeyError(name)


def per_px(v, Mg):
    """[G][C] -> [M][C]"""
    return v.repeat_interleave(Mg, 0)


def rnd(x, dt):
    """Rounded to the storage type (dt None: float64 arithmetic throughout, for the autograd comparison)."""
    return x if dt is None else x.to(dt).double()


def half_ulp(ref, dt):
    """Half a storage ulp of ``ref`` (subnormal spacing below the smallest normal)."""
    mant, emin = (7, -126) if dt is torch.bfloat16 else (10, -14)
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** emin)))
    return 0.5 * 2.0 ** (e - mant)


# ------------------------------------------------------------------ finalize
def ref_finalize(stats, G, C, Mtot, gamma, beta, rm, rv, mom=MOM, eps=EPS):
    """stats [G][T][2][C] (or None: eval mode), float64.  Returns a dict: mean, invstd, scale, shift
    [G][C]; parked [G][2][C] (mean, biased variance) in training mode; rm, rv after the G updates and
    rbound_m, rbound_v = sum over the updates of 2^-22 (|old| + |new|) where running statistics were given."""
    out = {}
    if stats is None:
        mu = (rm if rm is not None else torch.zeros(C, dtype=torch.float64, device=gamma.device)).expand(G, C)
        var = (rv if rv is not None else torch.ones(C, dtype=torch.float64, device=gamma.device)).expand(G, C)
    else:
        Mg = Mtot // G
        s = stats.sum(1)
        mu = s[:, 0] / Mg
        var = (s[:, 1] / Mg - mu * mu).clamp_min(0)
        out["parked"] = torch.stack([mu, var], 1)
        if rm is not None:
            unb = var * Mg / (Mg - 1) if Mg > 1 else var
            m, v = rm.clone(), rv.clone()
            bm, bv = torch.zeros_like(m), torch.zeros_like(v)
            for g in range(G):
                bm += 2.0 ** -22 * ((1 - mom) * m.abs() + mom * mu[g].abs())
                bv += 2.0 ** -22 * ((1 - mom) * v.abs() + mom * unb[g].abs())
                m = (1 - mom) * m + mom * mu[g]
                v = (1 - mom) * v + mom * unb[g]
            out.update(rm=m, rv=v, rbound_m=bm, rbound_v=bv)
    inv = 1.0 / torch.sqrt(var + eps)
    out.update(mean=mu, invstd=inv, scale=gamma * inv, shift=beta - mu * (gamma * inv))
    return out


def ref_bwd_finalize(sums, G, C, Mtot, gamma, mean, invstd):
    """sums [G][2][C] = (sum g, sum g*xhat).  coef [G][3][C] of dy = A g + B y + C, the absolute terms of
    the C row, dgamma and dbeta (summed over the groups)."""
    Mg = Mtot // G
    s1, s2 = sums[:, 0], sums[:, 1]
    A = gamma * invstd
    B = -A * invstd * s2 / Mg
    t1, t2 = -A * s1 / Mg, A * invstd * mean * s2 / Mg
    return {"coef": torch.stack([A, B, t1 + t2], 1), "cabs": t1.abs() + t2.abs(), "dgamma": s2.sum(0),
            "dbeta": s1.sum(0)}


# ------------------------------------------------------------------ forward
def ref_act(y, scale, shift, Mg, relu, res=None, rscale=None, rshift=None):
    """act(y*scale + shift [+ res | + res*rscale + rshift]) unrounded, the sum of the absolute terms and
    the number k of fp32 operations behind an element."""
    sc, sh = per_px(scale, Mg), per_px(shift, Mg)
    t, ab, k = y * sc + sh, (y * sc).abs() + sh.abs(), 2
    if res is not None and rscale is None:
        t, ab, k = t + res, ab + res.abs(), 3
    elif res is not None:
        rs, rh = per_px(rscale, Mg), per_px(rshift, Mg)
        t, ab, k = t + (res * rs + rh), ab + (res * rs).abs() + rh.abs(), 5
    return (t.clamp_min(0) if relu else t), ab, k


def windows2(a, shape):
    """[M][C] -> [N][H/2][W/2][4][C], window position d = 2*dy + dx"""
    N, H, W, C, _ = shape
    return a.view(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, H // 2, W // 2, 4, C)


def unwindows2(w, shape):
    N, H, W, C, _ = shape
    return w.view(N, H // 2, W // 2, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N * H * W, C)


def ref_pool2(a, shape):
    """2x2 max pool of the ROUNDED activation a [M][C]: pooled [M/4][C] and, per pixel, whether it is its
    window's first maximum in d order."""
    win = windows2(a, shape)
    mx = win.max(3).values
    eq = win == mx.unsqueeze(3)
    first = eq & (eq.long().cumsum(3) == 1)
    return mx.reshape(-1, a.shape[1]), unwindows2(first, shape)


def ref_pool3_fwd(a, shape):
    """MaxPool(3, 2, 1) of the rounded activation a [M][C]: out [N*Ho*Wo][C] and argmax (uint8), the
    first maximum in dy*3 + dx order; padding never wins."""
    N, H, W, C, _ = shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = torch.full((N, 2 * Ho + 1, 2 * Wo + 1, C), -float("inf"), dtype=torch.float64, device=a.device)
    x[:, 1:H + 1, 1:W + 1] = a.view(N, H, W, C)
    best = torch.full((N, Ho, Wo, C), -float("inf"), dtype=torch.float64, device=a.device)
    am = torch.zeros((N, Ho, Wo, C), dtype=torch.uint8, device=a.device)
    for tap in range(9):
        cand = x[:, tap // 3:tap // 3 + 2 * Ho:2, tap % 3:tap % 3 + 2 * Wo:2]
        take = cand > best
        best = torch.where(take, cand, best)
        am = torch.where(take, torch.full_like(am, tap), am)
    return best.reshape(-1, C), am.reshape(-1, C)


def ref_pool3_bwd(argmax, dout, shape, dt):
    """Per pixel the sum of dout over the windows whose recorded argmax is the pixel (codes that point at
    padding contribute nothing), rounded to the storage type: [M][C]."""
    N, H, W, C, _ = shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    am, d = argmax.view(N, Ho, Wo, C).long(), dout.view(N, Ho, Wo, C)
    oy = torch.arange(Ho, device=am.device).view(1, Ho, 1, 1)
    ox = torch.arange(Wo, device=am.device).view(1, 1, Wo, 1)
    iy, ix = 2 * oy - 1 + am // 3, 2 * ox - 1 + am % 3
    ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    n = torch.arange(N, device=am.device).view(N, 1, 1, 1)
    c = torch.arange(C, device=am.device).view(1, 1, 1, C)
    flat = ((n * H + iy.clamp(0, H - 1)) * W + ix.clamp(0, W - 1)) * C + c
    g = torch.zeros(N * H * W * C, dtype=torch.float64, device=am.device)
    g.index_add_(0, flat.reshape(-1), torch.where(ok, d, torch.zeros_like(d)).reshape(-1))
    return rnd(g.view(N * H * W, C), dt)


# ------------------------------------------------------------------ backward
def mask_slack(y, scale, shift, Mg):
    """(y*scale + shift, the fp32 slack of that value: two operations on its absolute terms)"""
    sc, sh = per_px(scale, Mg), per_px(shift, Mg)
    return y * sc + sh, 2 * U23 * ((y * sc).abs() + sh.abs())


def ref_reduce(d, y, Mg, mean, invstd, mask, scale=None, shift=None, msrc=None, exact=True):
    """g = d masked (0 none, 1 y*scale + shift > 0 strictly, 2 msrc > 0) [M][C]; sums [G][2][C] =
    (sum g, sum g*xhat); their any-order bounds [G][2][C]; and ``open`` [M][C], the elements whose mask
    decision lies within the fp32 slack of zero (none with exact operands: there 0 is 0)."""
    G, C = mean.shape
    keep = torch.ones_like(d, dtype=torch.bool)
    open_ = torch.zeros_like(keep)
    if mask == 1:
        t, slack = mask_slack(y, scale, shift, Mg)
        keep = t > 0
        if not exact:
            open_ = t.abs() <= slack
    elif mask == 2:
        keep = msrc > 0
    g = torch.where(keep, d, torch.zeros_like(d))
    mu, is_ = per_px(mean, Mg), per_px(invstd, Mg)
    gx = g * (y - mu) * is_
    gxa = g.abs() * (y.abs() + mu.abs()) * is_
    fold = lambda v: v.view(G, Mg, C).sum(1)  # noqa: E731
    sums = torch.stack([fold(g), fold(gx)], 1)
    # a sum of Mg terms in any order, the second after three operations per term; an open element may
    # be in or out
    da = torch.where(open_, d.abs(), torch.zeros_like(d))
    ob = torch.stack([fold(da), fold(da * (y.abs() + mu.abs()) * is_)], 1)
    bound = torch.stack([Mg * U23 * fold(g.abs()), (Mg + 3) * U23 * fold(gxa)], 1) + ob
    return g, sums, bound, open_


def ref_apply(g, y, coef, Mg, mscale=None, mshift=None, exact=True):
    """dy = A*g' + B*y + C unrounded (g' = g, or g where y*mscale + mshift > 0), the absolute terms, the
    open elements, dbias = the column sums of the UNROUNDED dy (the kernel adds the fp32 values before it
    packs them) and its any-order bound."""
    open_ = torch.zeros_like(g, dtype=torch.bool)
    if mscale is not None:
        t, slack = mask_slack(y, mscale, mshift, Mg)
        if not exact:
            open_ = t.abs() <= slack
        g = torch.where(t > 0, g, torch.zeros_like(g))
    A, B, Cc = (per_px(coef[:, i], Mg) for i in range(3))
    dy = A * g + B * y + Cc
    ab = (A * g).abs() + (B * y).abs() + Cc.abs()
    M = g.shape[0]
    return dy, ab, open_, dy.sum(0), (M + 4) * U23 * ab.sum(0)


def granules(terms, granule):
    """Largest column sum of |terms| in units of ``granule``: below 2^24, every partial sum of the terms
    is an integer number of granules that fp32 holds exactly, in any order."""
    return float(terms.abs().reshape(-1, terms.shape[-1]).sum(0).max() / granule)


# ------------------------------------------------------------------ buffers
class Slice16:
    """[M][C] 16-bit at channel OFF of [M + 2*img][C + PAD] (dense: [C]) NaN; one NaN image before and one
    after.  ``value`` None: an output, NaN throughout."""

    def __init__(self, value, M, C, img, dt, dev, wide=True):
        self.cs, self.off, self.M, self.C, self.img = (C + PAD, OFF, M, C, img) if wide else (C, 0, M, C, img)
        self.buf = torch.full((M + 2 * img, self.cs), float("nan"), dtype=dt, device=dev)
        if value is not None:
            stored = value.to(dt)
            assert torch.equal(stored.double(), value), "operand not exact in the storage type"
            self.buf[img:img + M, self.off:self.off + C] = stored
        self.ptr = self.buf.data_ptr() + 2 * (img * self.cs + self.off)

    def get(self):
        return self.buf[self.img:self.img + self.M, self.off:self.off + self.C].double()

    def untouched_outside(self):
        m = torch.ones_like(self.buf, dtype=torch.bool)
        m[self.img:self.img + self.M, self.off:self.off + self.C] = False
        return bool(torch.isnan(self.buf[m]).all())


class F32:
    """n floats (``value`` or NaN) between GUARD sentinel floats each side."""

    def __init__(self, value, n, dev):
        self.n = n
        self.bits = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        self.mid = self.bits[GUARD:GUARD + n].view(torch.float32)
        if value is None:
            self.mid.fill_(float("nan"))
        else:
            v32 = value.reshape(-1).float()
            assert torch.equal(v32.double(), value.reshape(-1).double()), "operand not exact in fp32"
            self.mid.copy_(v32)
        self.ptr = self.mid.data_ptr()

    def get(self):
        return self.mid.double()

    def guards_intact(self):
        return bool((self.bits[:GUARD] == SENTINEL).all() and (self.bits[GUARD + self.n:] == SENTINEL).all())
