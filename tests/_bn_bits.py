"""Cases and digests of tests/golden/bn_bits.json (shared by its generator and its test).

A case is one BatchNorm C entry point (include/stfunet.h), a shape (N, H, W, C, groups) and an
option set; its inputs come from ``numpy.random.default_rng(crc32(case id))``.  The 16-bit tensors
(y, dz, dpool, residual, mask source) hold multiples of 0.25 in [-2, 2] -- exact in bf16 and fp16,
and few enough values that 2x2 windows contain exact ties -- and are channel slices (offset 8) of
buffers 16 channels wider than C wherever the entry point takes a channel stride; the fp32 vectors
(scale, shift, mean, invstd, coef) are not quantised, so a changed contraction or summation order
shows.  ``run`` calls the entry point once and returns every output buffer (pre-filled with NaN,
the wide ones whole, so an unwritten or a stray element shows); ``digests`` is their SHA-256.

``REF`` cases also have a float64 CPU restatement (``ref_errors``): the generic ``stf_bn_act`` kernel
(C = 24) and the one-thread-per-window pooled reduce (C = 1024), which no other test reaches.
"""
import hashlib
import zlib

import numpy as np
import torch

PAD, OFF = 16, 8                       # wide buffers: C + PAD channels, the slice starts at OFF
REF_BOUND = 1e-2                       # rel-L2, the bound tests/test_kernels_gpu.py uses for BN
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}

UNPOOLED = [(4, 5, 7, 64, 2), (2, 3, 3, 8, 1), (1, 2, 2, 2048, 1)]
GENERIC = (2, 3, 5, 24, 1)             # C / 8 = 3 divides no block: stf_bn_act's generic kernel
POOL_DPP = [(4, 6, 10, 64, 2), (2, 4, 4, 512, 1)]
POOL_WINDOW = (2, 4, 4, 1024, 1)       # 64 % (C / 8) != 0: one thread per window
POOL3 = [(2, 9, 11, 64, 2), (2, 8, 8, 64, 1)]


def cases():
    """[(entry point, shape, options)]; options is a tuple of (name, value) pairs."""
    out = [(e, (0, 0, 0, 64, g), ()) for e in ("finalize", "bwd_finalize") for g in (1, 3)]
    for s in UNPOOLED + [GENERIC]:
        out += [("act", s, (("res", r), ("relu", a))) for r in (0, 1, 2) for a in (0, 1)]
    for s in (POOL_DPP[0], POOL_WINDOW):
        out += [("act_pool", s, (("relu", a),)) for a in (0, 1)]
    for s in UNPOOLED:
        out += [("reduce", s, (("mask", m), ("g_out", g))) for m in (0, 1, 2) for g in (1, 0)]
    for s in POOL_DPP + [POOL_WINDOW]:
        out += [("reduce_pool", s, (("dz", d), ("mask", m))) for d in (1, 0) for m in (0, 1)]
    for s in UNPOOLED:
        out += [("apply", s, (("mask", m), ("bias", b))) for m in (0, 1) for b in (0, 1)]
    for s in POOL3:
        out += [("reduce_pool3", s, ()), ("apply_pool3", s, ())]
    return out


def case_id(entry, shape, opts):
    return "-".join([entry, "x".join(str(v) for v in shape)] + [f"{k}{v}" for k, v in opts])


def is_ref(entry, shape, opts):
    return (entry == "act" and shape == GENERIC) or (entry == "reduce_pool" and shape == POOL_WINDOW)


def seed_of(entry, shape, opts):
    return zlib.crc32(case_id(entry, shape, opts).encode())


class _Gen:
    """The seeded inputs of one case, generated on the CPU and kept there for ``ref_errors``."""

    def __init__(self, seed, dtype, dev):
        self.rng, self.dtype, self.dev, self.cpu = np.random.default_rng(seed), dtype, dev, {}

    def q16(self, name, M, C, wide=True, nonneg=False):
        """[M][C] multiples of 0.25 in [-2, 2]; returns the device tensor that holds it (wide: the
        slice's surroundings hold such values too) and its channel stride."""
        cs = C + PAD if wide else C
        v = torch.from_numpy(self.rng.integers(0 if nonneg else -8, 9, (M, cs)).astype(np.float32) / 4)
        self.cpu[name] = v[:, OFF:OFF + C].double() if wide else v.double()
        return v.to(self.dtype).to(self.dev), cs

    def f32(self, name, n, lo, hi):
        v = torch.from_numpy(self.rng.uniform(lo, hi, n).astype(np.float32))
        self.cpu[name] = v.double()
        return v.to(self.dev)

    def nan16(self, M, C, wide=True):
        cs = C + PAD if wide else C
        return torch.full((M, cs), float("nan"), dtype=self.dtype, device=self.dev), cs

    def nan32(self, n):
        return torch.full((n,), float("nan"), device=self.dev)


def _ptr(t, wide=True):
    return t.data_ptr() + (OFF * 2 if wide else 0)


def run(entry, shape, opts, dtype, dev="cuda"):
    """One call of the case's entry point in ``dtype``'s library: ({name: output tensor}, inputs on
    the CPU as float64 for ``ref_errors``)."""
    from stfunet import _lib
    from stfunet._lib import call, stream
    N, H, W, C, G = shape
    o = dict(opts)
    g = _Gen(seed_of(entry, shape, opts), dtype, dev)
    M = N * H * W
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    with _lib.storage(dtype):
        lib = _lib.load()
        if entry == "finalize":
            T, Mtot = 37, 3000
            stats = torch.from_numpy(g.rng.standard_normal((G, T, 2, C)).astype(np.float32) * 10)
            stats[:, :, 1] = stats[:, :, 1].abs() + 30
            stats = stats.to(dev)
            gamma, beta = g.f32("gamma", C, -1.5, 1.5), g.f32("beta", C, -0.5, 0.5)
            rm, rv = g.f32("rm", C, -0.5, 0.5), g.f32("rv", C, 0.5, 2.0)
            outs = {k: g.nan32(G * C) for k in ("mean", "invstd", "scale", "shift")}
            call("stf_bn_finalize", p(stats), T, G, C, Mtot, p(gamma), p(beta), 0.1, 1e-5, p(rm), p(rv),
                 p(outs["mean"]), p(outs["invstd"]), p(outs["scale"]), p(outs["shift"]), stream())
            outs.update(running_mean=rm, running_var=rv)
        elif entry == "bwd_finalize":
            T, Mtot = 37, 3000
            part = torch.from_numpy(g.rng.standard_normal((G, T, 2, C)).astype(np.float32)).to(dev)
            gamma, mean = g.f32("gamma", C, -1.5, 1.5), g.f32("mean", G * C, -0.5, 0.5)
            invstd = g.f32("invstd", G * C, 0.5, 2.0)
            outs = {"dgamma": g.nan32(C), "dbeta": g.nan32(C), "coef": g.nan32(G * 3 * C)}
            call("stf_bn_bwd_finalize", p(part), T, G, C, Mtot, p(gamma), p(mean), p(invstd), p(outs["dgamma"]),
                 p(outs["dbeta"]), p(outs["coef"]), stream())
        elif entry in ("act", "act_pool"):
            y, ycs = g.q16("y", M, C)
            scale, shift = g.f32("scale", G * C, -1.5, 1.5), g.f32("shift", G * C, -0.5, 0.5)
            res, rcs, rs, rh = None, 0, None, None
            if o.get("res"):
                res, rcs = g.q16("res", M, C)
                if o["res"] == 2:
                    rs, rh = g.f32("rscale", G * C, -1.5, 1.5), g.f32("rshift", G * C, -0.5, 0.5)
            out, ocs = g.nan16(M, C)
            outs = {"out": out}
            pooled = None
            if entry == "act_pool":
                pooled, _ = g.nan16(M // 4, C, wide=False)
                outs["pooled"] = pooled
            call("stf_bn_act", _ptr(y), ycs, N, H, W, C, G, p(scale), p(shift), o["relu"],
                 None if res is None else _ptr(res), rcs, p(rs), p(rh), _ptr(out), ocs, p(pooled), stream())
        elif entry in ("reduce", "reduce_pool"):
            pool = entry == "reduce_pool"
            y, ycs = g.q16("y", M, C)
            dz, dzcs = g.q16("dz", M, C) if o.get("dz", 1) else (None, 0)
            dpool = g.q16("dpool", M // 4, C, wide=False)[0] if pool else None
            scale, shift = g.f32("scale", G * C, -1.5, 1.5), g.f32("shift", G * C, -0.5, 0.5)
            mean, invstd = g.f32("mean", G * C, -0.5, 0.5), g.f32("invstd", G * C, 0.5, 2.0)
            msrc, mcs = g.q16("msrc", M, C, nonneg=True) if o["mask"] == 2 else (None, 0)
            tpg = lib.stf_bn_bwd_tiles(N, H, W, C, G, int(pool))
            outs = {"partial": g.nan32(G * tpg * 2 * C)}
            if o.get("g_out", 1):
                outs["g_out"] = g.nan16(M, C, wide=False)[0]
            call("stf_bn_bwd_reduce", None if dz is None else _ptr(dz), dzcs, p(dpool), _ptr(y), ycs, N, H, W, C,
                 G, p(scale), p(shift), p(mean), p(invstd), o["mask"], None if msrc is None else _ptr(msrc), mcs,
                 p(outs.get("g_out")), p(outs["partial"]), stream())
        elif entry == "apply":
            gin, gcs = g.q16("g", M, C)
            y, ycs = g.q16("y", M, C)
            coef = g.f32("coef", G * 3 * C, -1.0, 1.0)
            ms = mh = None
            if o["mask"]:
                ms, mh = g.f32("scale", G * C, -1.5, 1.5), g.f32("shift", G * C, -0.5, 0.5)
            dy, dycs = g.nan16(M, C)
            outs = {"dy": dy}
            bp = None
            if o["bias"]:
                bp = g.nan32(lib.stf_bn_bwd_apply_tiles(M, C) * C)      # scratch: consumed by the call
                outs["dbias"] = g.nan32(C)
            call("stf_bn_bwd_apply", _ptr(gin), gcs, _ptr(y), ycs, M, C, G, p(ms), p(mh), p(coef), _ptr(dy), dycs,
                 p(bp), p(outs.get("dbias")), stream())
        elif entry in ("reduce_pool3", "apply_pool3"):
            Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
            argmax = torch.from_numpy(g.rng.integers(0, 9, (N * Ho * Wo, C)).astype(np.uint8)).to(dev)
            dout = g.q16("dout", N * Ho * Wo, C, wide=False)[0]
            y = g.q16("y", M, C, wide=False)[0]
            scale, shift = g.f32("scale", G * C, -1.5, 1.5), g.f32("shift", G * C, -0.5, 0.5)
            if entry == "reduce_pool3":
                mean, invstd = g.f32("mean", G * C, -0.5, 0.5), g.f32("invstd", G * C, 0.5, 2.0)
                outs = {"partial": g.nan32(G * lib.stf_bn_bwd_tiles(N, H, W, C, G, 0) * 2 * C)}
                call("stf_bn_bwd_reduce_pool3", p(argmax), p(dout), p(y), N, H, W, C, G, p(scale), p(shift), p(mean),
                     p(invstd), p(outs["partial"]), stream())
            else:
                coef = g.f32("coef", G * 3 * C, -1.0, 1.0)
                outs = {"dy": g.nan16(M, C, wide=False)[0]}
                call("stf_bn_bwd_apply_pool3", p(argmax), p(dout), p(y), N, H, W, C, G, p(scale), p(shift), p(coef),
                     p(outs["dy"]), stream())
        else:
            raise ValueError(entry)
    torch.cuda.synchronize()
    return outs, g.cpu


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def digests(entry, shape, opts, dtype, dev="cuda"):
    return {k: _sha(v) for k, v in run(entry, shape, opts, dtype, dev)[0].items()}


def _rel(a, b):
    return float((a.double() - b).norm() / b.norm().clamp_min(1e-30))


def ref_errors(entry, shape, opts, dtype, outs, cpu):
    """{output: rel-L2 against float64 on the CPU} of a ``is_ref`` case (``outs``, ``cpu`` from ``run``)."""
    N, H, W, C, G = shape
    o = dict(opts)
    per_px = lambda v: v.view(G, 1, C).expand(G, N * H * W // G, C).reshape(-1, C)  # noqa: E731
    a = cpu["y"] * per_px(cpu["scale"]) + per_px(cpu["shift"])
    if entry == "act":
        if o["res"] == 1:
            a = a + cpu["res"]
        elif o["res"] == 2:
            a = a + cpu["res"] * per_px(cpu["rscale"]) + per_px(cpu["rshift"])
        if o["relu"]:
            a = a.clamp_min(0)
        return {"out": _rel(outs["out"].cpu()[:, OFF:OFF + C], a)}
    # pooled reduce: the 2x2 window's first maximum of the 16-bit-rounded activation takes dpool
    act = (a.clamp_min(0) if o["mask"] == 1 else a).to(dtype).double().view(N, H // 2, 2, W // 2, 2, C)
    win = act.permute(0, 1, 3, 2, 4, 5).reshape(N, H // 2, W // 2, 4, C)          # d = 2 * dy + dx
    eq = (win == win.max(3, keepdim=True).values).double()
    first = eq * (eq.cumsum(3) == 1)
    routed = first * cpu["dpool"].view(N, H // 2, W // 2, 1, C)
    gr = routed.view(N, H // 2, W // 2, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, C)
    if o["dz"]:
        gr = gr + cpu["dz"]
    if o["mask"] == 1:
        gr = gr * (a > 0)
    xhat = (cpu["y"] - per_px(cpu["mean"])) * per_px(cpu["invstd"])
    sums = torch.stack([gr.view(G, -1, C).sum(1), (gr * xhat).view(G, -1, C).sum(1)], 1)     # [G][2][C]
    got = outs["partial"].cpu().double().view(G, -1, 2, C).sum(1)
    return {"g_out": _rel(outs["g_out"].cpu(), gr), "partial": _rel(got, sums)}
