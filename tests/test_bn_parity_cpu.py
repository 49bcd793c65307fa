"""The BatchNorm parity reference (tests/_bn_ref.py) is right, and its case table means what it says.

No GPU: (1) the float64 reference chain reduce -> bwd_finalize -> apply (with finalize and act in front)
agrees with torch autograd of F.batch_norm(training=True) + ReLU, with the residual add, max_pool2d(2) and
max_pool2d(3, 2, 1), per group as G sequential calls of one nn.BatchNorm2d, to 1e-11; (2) every case of
the table has the edge it is listed for, from the shape and csrc/bn.hip's constants and from the host-only
queries stf_bn_bwd_tiles / stf_bn_bwd_apply_tiles; (3) the exact run's operands are exact: the reference
recomputed stepwise in float32 left to right, with every multiply-add fused, and with every sum reversed
equals the float64 result, and every compared sum stays below 2^24 granules; the Gaussian operands leave
at most 1e-4 of a case's elements with an open mask decision.
"""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bn_ref as R

DTYPES = [torch.bfloat16, torch.float16]
f64 = torch.float64


# ------------------------------------------------------------------ 1. against autograd
def nchw(t, shape):
    N, H, W, C, _ = shape
    return t.view(N, H, W, C).permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


CHAIN_SHAPES = [(6, 6, 10, 16, 3), (4, 5, 7, 8, 1), (4, 2, 3, 8, 2)]      # (a group of 2 pixels cancels to 1e-3 of its terms)


@pytest.mark.parametrize("variant,shape", [(v, s) for v in ("plain", "norelu", "res", "pool2", "pool3")
                                           for s in CHAIN_SHAPES if v != "pool2" or not (s[1] % 2 or s[2] % 2)], ids=str)
def test_reference_chain_is_autograd(variant, shape):
    N, H, W, C, G = shape
    M, Mg, Ng = N * H * W, N * H * W // G, N // G
    gen = torch.Generator().manual_seed(zlib.crc32(repr((variant, shape)).encode()))
    rn = lambda *s: torch.randn(s, generator=gen, dtype=f64)  # noqa: E731
    y, res, gamma, beta = rn(M, C) * 1.5 + 0.3, rn(M, C), rn(C), rn(C)
    rm0, rv0 = rn(C), rn(C).abs() + 0.5
    # torch: G sequential calls of one module
    bn = torch.nn.BatchNorm2d(C, eps=R.EPS, momentum=R.MOM).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rm0), bn.running_var.copy_(rv0)
    yt = nchw(y, shape).clone().requires_grad_(True)
    z = torch.cat([bn(yt[g * Ng:(g + 1) * Ng]) for g in range(G)], 0)
    if variant == "res":
        z = z + nchw(res, shape)
    a = z if variant == "norelu" else F.relu(z)
    w_a = nchw(rn(M, C), shape)
    if variant == "pool2":
        p = F.max_pool2d(a, 2)
        w_p = torch.randn(p.shape, generator=gen, dtype=f64)
        loss = (a * w_a).sum() + (p * w_p).sum()
    elif variant == "pool3":
        p = F.max_pool2d(a, 3, 2, 1)
        w_p = torch.randn(p.shape, generator=gen, dtype=f64)
        loss = (p * w_p).sum()
    else:
        loss = (a * w_a).sum()
    loss.backward()
    # the reference: statistics rows -> finalize -> act -> reduce -> bwd_finalize -> apply
    yg = y.view(G, Mg, C)
    stats = torch.stack([yg.sum(1), (yg * yg).sum(1)], 1).view(G, 1, 2, C)
    fin = R.ref_finalize(stats, G, C, M, gamma, beta, rm0, rv0)
    relu = variant != "norelu"
    out, _, _ = R.ref_act(y, fin["scale"], fin["shift"], Mg, relu, res if variant == "res" else None)
    assert torch.allclose(out, nhwc(a.detach()), rtol=1e-11, atol=1e-11)
    d, mask, msrc = nhwc(w_a), int(relu), None
    if variant == "res":
        mask, msrc = 2, out
    elif variant == "pool2":
        pooled, first = R.ref_pool2(out, shape)
        assert torch.allclose(pooled, nhwc(p.detach()), rtol=1e-11, atol=1e-11)
        routed = R.unwindows2(R.windows2(first.double(), shape) * nhwc(w_p).view(N, H // 2, W // 2, 1, C), shape)
        d = d + routed
    elif variant == "pool3":
        pooled, am = R.ref_pool3_fwd(out, shape)
        assert torch.allclose(pooled, nhwc(p.detach()), rtol=1e-11, atol=1e-11)
        d = R.ref_pool3_bwd(am, nhwc(w_p), shape, None)
    g, sums, _, _ = R.ref_reduce(d, y, Mg, fin["mean"], fin["invstd"], mask, fin["scale"], fin["shift"], msrc)
    bf = R.ref_bwd_finalize(sums, G, C, M, gamma, fin["mean"], fin["invstd"])
    dy = R.ref_apply(g, y, bf["coef"], Mg)[0]
    rel = lambda a_, b_: float((a_ - b_).abs().max() / b_.abs().max().clamp_min(1e-300))  # noqa: E731
    assert rel(dy, nhwc(yt.grad)) < 1e-11
    assert rel(bf["dgamma"], bn.weight.grad) < 1e-11 and rel(bf["dbeta"], bn.bias.grad) < 1e-11
    assert rel(fin["rm"], bn.running_mean) < 1e-11 and rel(fin["rv"], bn.running_var) < 1e-11
    # the recomputed-mask form of apply gives the same dy from the unmasked gradient
    if mask == 1:
        dy2 = R.ref_apply(d, y, bf["coef"], Mg, fin["scale"], fin["shift"])[0]
        assert torch.equal(dy2, dy)


def test_finalize_reference_corners():
    C, G = 8, 2
    gamma, beta = torch.arange(1, C + 1, dtype=f64), torch.ones(C, dtype=f64)
    # Mg = 1: the biased variance goes into the running update; a negative variance is clamped to 0
    stats = torch.tensor([3.0, 9.0], dtype=f64).view(1, 1, 2, 1).expand(G, 1, 2, C).clone()
    stats[1, 0, 1] = 8.0                                    # sum of squares below mean^2: variance -1
    fin = R.ref_finalize(stats, G, C, G, gamma, beta, torch.zeros(C, dtype=f64), torch.ones(C, dtype=f64))
    assert torch.equal(fin["parked"][:, 1], torch.zeros(G, C, dtype=f64))
    assert torch.allclose(fin["invstd"], torch.full((G, C), R.EPS ** -0.5, dtype=f64))
    assert torch.allclose(fin["rv"], torch.full((C,), (1 - R.MOM) ** 2, dtype=f64))
    # eval mode: running statistics, or 0 / 1 without them; nothing advances
    ev = R.ref_finalize(None, G, C, 10, gamma, beta, None, None)
    assert "rm" not in ev and torch.equal(ev["mean"], torch.zeros(G, C, dtype=f64))
    assert torch.allclose(ev["scale"], (gamma / (1 + R.EPS) ** 0.5).expand(G, C))


# ------------------------------------------------------------------ 2. every case has its edge
def libs():
    from stfunet import _lib
    return [_lib.load(dt) for dt in DTYPES]


def units(shape):
    N, H, W, C, G = shape
    return N * H * W // G * (C // 8)


@pytest.mark.parametrize("shape,edge", R.GROUP_MAJOR, ids=str)
def test_group_major_edges(shape, edge):
    N, H, W, C, G = shape
    upg, M = units(shape), N * H * W
    assert R.cg_ok(C) and N % G == 0
    for lib in libs():
        tpg = lib.stf_bn_bwd_tiles(N, H, W, C, G, 0)
        btiles = lib.stf_bn_bwd_apply_tiles(M, C)
        assert tpg == R.reduce_tiles(upg, G) and btiles == min(R.ROW_CAP, max(1, -(-M * (C // 8) // R.NT)))
        act_t, bias_t = R.g_tiles(upg, G, R.ACT_CAP), R.g_tiles(upg, G, btiles)
        per_iter = R.NT * R.UPT
        if edge == "below_block":
            assert upg < R.NT and tpg == 1 and act_t == 1
        elif edge == "ragged_idle":
            busy = -(-upg // per_iter)
            assert act_t == busy >= 2 and tpg > busy                 # several blocks per group; idle reduce blocks
            assert 0 < upg - (busy - 1) * per_iter <= R.NT           # the last block ends inside its first chunk
        else:
            for t in (tpg, bias_t):                                   # the capped grids: reduce, apply with bias sums
                assert t * G <= R.ROW_CAP and t < -(-upg // per_iter)         # capped below what the units ask for
                assert 0 < upg - t * per_iter < per_iter                      # second iteration: one ragged block
    assert {s[3] for s, _ in R.GROUP_MAJOR} == {8, 64, 2048}


def test_big_case_passes_the_block_cap():
    N, H, W, C, G = R.BIG
    upg = units(R.BIG)
    assert R.cg_ok(C) and R.g_tiles(upg, G, R.ACT_CAP) == R.ACT_CAP
    rest = upg - R.ACT_CAP * R.NT * R.UPT
    assert 0 < rest < R.ACT_CAP * R.NT * R.UPT and rest % (R.NT * R.UPT) % R.NT != 0      # second iteration, ragged


def test_generic_and_pooled_edges():
    for s in R.GENERIC:
        assert s[3] % 8 == 0 and not R.cg_ok(s[3])
    assert {s[3] for s in R.GENERIC} == {24, 4096} and any(s[4] == 3 and s[3] == 4096 for s in R.GENERIC)
    assert any(s[4] > 1 for s in R.GENERIC)
    for s in R.POOL_ACT:
        assert (s[1] // 2) % 2 == 1 and (s[2] // 2) % 2 == 1 and s[1] % 2 == 0 and s[2] % 2 == 0 and s[4] > 1
    assert {s[3] for s in R.POOL_ACT} == {8, 64, 1024}
    assert {s[3] for s, _ in R.POOL_DPP} == {8, 64, 512} and {s[3] for s, _ in R.POOL_WIN} == {1024, 2048}
    for lib in libs():
        for (N, H, W, C, G), edge in R.POOL_DPP + R.POOL_WIN:
            CG = C // 8
            upg = N // G * (H // 2) * (W // 2) * CG
            tpg = lib.stf_bn_bwd_tiles(N, H, W, C, G, 1)
            assert tpg == R.reduce_tiles(upg, G) and R.cg_ok(C)
            assert (64 % CG == 0) == edge.startswith("dpp")
            if edge == "dpp_unpaired":                   # a second iteration whose paired unit is absent
                U, S = 4 * upg, tpg * R.PNT
                assert 2 * S < U <= 3 * S
            if edge == "win":
                assert (tpg * R.NT) % CG == 0


def test_pool3_edges():
    shapes = [s for s, _ in R.POOL3]
    assert any(s[1] == 1 for s in shapes) and any(s[2] == 1 for s in shapes)
    assert any(s[1] == 2 for s in shapes) and any(s[2] == 2 for s in shapes)
    assert any(s[1] % 2 and s[2] % 2 and s[1] > 2 for s in shapes) and any(s[1] % 2 == 0 and s[2] % 2 == 0 for s in shapes)
    assert any(s[4] > 1 for s in shapes)
    for lib in libs():
        for (N, H, W, C, G), edge in R.POOL3:
            assert R.cg_ok(C)
            tpg = lib.stf_bn_bwd_tiles(N, H, W, C, G, 0)
            assert tpg == R.reduce_tiles(units((N, H, W, C, G)), G)
            blocks2 = N // G * ((H + 1) // 2) * ((W + 1) // 2) * (C // 8)
            assert (blocks2 > 2 * tpg * R.NT) == (edge == "pool3_second")     # two units per thread and iteration


def test_finalize_edges():
    assert {t for t, _, _ in R.FINALIZE} == {1, 37, 1024, 1025, 5000}
    assert {c for _, c, _ in R.FINALIZE} == {8, 24, 64, 2048} and {g for _, _, g in R.FINALIZE} == {1, 3}
    assert sum(t > R.ROW_CAP for t, _, _ in R.FINALIZE) >= 2 and any(t == R.ROW_CAP for t, _, _ in R.FINALIZE)
    for t in (1025, 5000):                                           # the pre-fold runs with one and with several groups
        assert {g for tt, _, g in R.FINALIZE if tt == t} == {1, 3}
    assert all(n > R.RUN_BATCH for n in R.BATCH_COUNTS) and max(R.BATCH_COUNTS) > 2 * R.RUN_BATCH


# ------------------------------------------------------------------ 3. exact operands are exact
def f32_three_ways(terms_fn, rows):
    """The column sums of ``terms_fn(fused)`` [rows][C] in float32: left to right, fused, reversed."""
    outs = []
    for fused, rev in ((False, False), (True, False), (False, True)):
        t = terms_fn(fused).numpy().astype(np.float32)
        if rev:
            t = t[::-1]
        acc = np.zeros(t.shape[1], np.float32)
        for r in range(rows):
            acc = (acc + t[r]).astype(np.float32)
        outs.append(torch.from_numpy(acc.astype(np.float64)))
    return outs


def fma(a, b, c, fused):
    """a*b + c in float32: one rounding when fused (the float32 product is exact in float64), else two."""
    a, b, c = a.float(), b.float(), c.float()
    if fused:
        return (a.double() * b.double() + c.double()).float()
    return a * b + c


@pytest.mark.parametrize("shape", [s for s, _ in R.GROUP_MAJOR[:4]] + [R.POOL_DPP[3][0], R.POOL3[5][0]], ids=str)
def test_exact_operands_are_exact_in_float32(shape):
    N, H, W, C, G = shape
    M, Mg = N * H * W, N * H * W // G
    o = R.Ops(shape, "exact", torch.bfloat16)
    y, dz = o["y"], o["dz"]
    d = dz + (o["g"] if H % 2 == 0 and W % 2 == 0 else 0)             # a routed 2x2 gradient at most doubles dz
    if shape == R.POOL3[5][0]:
        d = R.ref_pool3_bwd(o["argmax_rand"], o["dout"], shape, torch.bfloat16)
    sc, sh, mu, is_ = (R.per_px(o[k], Mg) for k in ("scale", "shift", "mean", "invstd"))
    # forward: y*scale + shift [+ res*rscale + rshift], exact in both storage types
    rs, rh = R.per_px(o["rscale"], Mg), R.per_px(o["rshift"], Mg)
    ref = R.ref_act(y, o["scale"], o["shift"], Mg, 0, o["res"], o["rscale"], o["rshift"])[0]
    for fused in (False, True):
        t = fma(y, sc, sh, fused) + fma(o["res"], rs, rh, fused)
        assert torch.equal(t.double(), ref)
    for dt in DTYPES:
        assert torch.equal(ref.to(dt).double(), ref)
    zero = float(((y * sc + sh) == 0).double().mean())
    assert zero > 0.01, zero                                          # the strict '>' is exercised
    # reduce: sum g, sum g * (y - mean) * invstd per group
    g, sums, _, open_ = R.ref_reduce(d, y, Mg, o["mean"], o["invstd"], 1, o["scale"], o["shift"])
    assert not open_.any()
    assert R.granules((g * (y - mu) * is_).view(G, Mg, C).abs().sum(1), 1 / 32) < 2 ** 24
    gsel = 0 if G == 1 else G - 1
    sl = slice(gsel * Mg, (gsel + 1) * Mg)
    for got in f32_three_ways(lambda fused: (g[sl].float() * (y[sl].float() - mu[sl].float())) * is_[sl].float(), Mg):
        assert torch.equal(got, sums[gsel, 1])
    # apply: dy = A*g + B*y + C and its column sums over all M
    coef = o["coef"]
    dy, ab, _, dbias, _ = R.ref_apply(g, y, coef, Mg)
    A, B, Cc = (R.per_px(coef[:, i], Mg) for i in range(3))
    for fused in (False, True):
        assert torch.equal((fma(A, g, fma(B, y, Cc, fused), fused)).double(), dy)
        assert torch.equal((fma(B, y, Cc, fused) + A.float() * g.float()).double(), dy)
    for dt in DTYPES:
        assert torch.equal(dy.to(dt).double(), dy)
    assert R.granules(dy.abs().sum(0, keepdim=True), 1 / 32) < 2 ** 24
    if M <= 20000:
        for got in f32_three_ways(lambda fused: fma(A, g, fma(B, y, Cc, fused), fused), M):
            assert torch.equal(got, dbias)


def test_dbias_of_the_listed_shape_passes_the_granule_limit():
    # why the exact run compares that dbias under the bounded rule: M terms of (on average) > 16 granules
    for shape in R.DBIAS_BOUNDED:
        assert shape[0] * shape[1] * shape[2] * 16 > 2 ** 24


def test_exact_windows_hold_ties():
    shape = R.POOL_DPP[1][0]
    o = R.Ops(shape, "exact", torch.bfloat16)
    Mg = shape[0] * shape[1] * shape[2] // shape[4]
    a = R.ref_act(o["y"], o["scale"], o["shift"], Mg, 1)[0]
    win = R.windows2(a, shape)
    ties = ((win == win.max(3, keepdim=True).values).sum(3) > 1).double().mean()
    assert ties > 0.2
    s3 = R.POOL3[0][0]
    o3 = R.Ops(s3, "exact", torch.bfloat16)
    a3 = R.ref_act(o3["y"], o3["scale"], o3["shift"], s3[0] * s3[1] * s3[2] // s3[4], 1)[0]
    out, am = R.ref_pool3_fwd(a3, s3)
    assert len(am.unique()) == 9 and out.min() >= 0                  # every tap wins somewhere; padding never


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_gaussian_operands_leave_few_open_masks(dt):
    for shape, _ in R.GROUP_MAJOR[:4]:
        o = R.Ops(shape, "gauss", dt)
        Mg = shape[0] * shape[1] * shape[2] // shape[4]
        t, slack = R.mask_slack(o["y"], o["scale"], o["shift"], Mg)
        assert float((t.abs() <= slack).double().mean()) <= 1e-4
