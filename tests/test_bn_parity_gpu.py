"""Every BatchNorm kernel of csrc/bn.hip and the fused stem pass of csrc/stf.hip against float64, per element.

The cases are tests/_bn_ref.py's table (tests/test_bn_parity_cpu.py checks the reference against torch
autograd and that every case has the edge it is there for), through the C entry points, in both storage
libraries.

Exact run: dyadic operands (see _bn_ref), so every fp32 intermediate is exact in any order, fused or not:
every 16-bit output must EQUAL the float64 reference rounded to the storage type, every summed partial
(its rows added in float64), dbias, dgamma and dbeta the exact sum.  A visible share of y*scale + shift is
exactly 0 (the strict '>' of the masks) and 2x2 / 3x3 windows hold ties (the first-maximum rule).
dbias is the column sum of the UNROUNDED fp32 dy: the kernel adds before it packs, and the reference
follows it.  One dbias passes 2^24 granules and is compared under the bounded rule (_bn_ref.DBIAS_BOUNDED).

Bounded run (unpooled entry points and the finalizes): Gaussian operands; a 16-bit output may differ from
the float64 reference by half a storage ulp plus k * 2^-23 * (sum of the absolute terms), k the fp32
operations behind the element; a sum of n terms by n * 2^-23 * sum |terms|; finalize outputs by 1 fp32
ulp (mean, invstd, coef rows -- of the absolute terms where a row is a difference), 2 ulp (scale),
2^-22 (|beta| + |mean*scale|) (shift) and 2^-22 (|old| + |new|) per running update.  An element whose
mask decision lies within the fp32 slack of zero is left out (at most 1e-4 of a case).  The finalizes'
statistics rows are integers in both runs wherever the in-place fp32 pre-fold runs (tiles > 1024), so the
fold itself is exact and the bounds above cover what follows it.  Each case prints its largest err / bound.

Buffers: every 16-bit tensor is a channel slice of a wider NaN buffer where the entry point takes a
stride, with a NaN image before and after; outputs start as NaN; fp32 buffers sit between sentinel words.
"""
import ctypes
import functools

import pytest
import torch

import _bn_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
KINDS = ["exact", "gauss"]
U23 = R.U23
WORST = {}                               # entry point -> largest err / bound of the bounded runs so far
f64 = torch.float64


def _id(v):
    return "bf16" if v is torch.bfloat16 else "fp16" if v is torch.float16 else str(v).replace(" ", "")


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=2)
def ops(shape, kind, dt, dev_gen=False):
    return R.Ops(shape, kind, dt, DEV, dev_gen)


def run(dt, name, *args):
    from stfunet import _lib
    with _lib.storage(dt):
        _lib.call(name, *args, _lib.stream())
    torch.cuda.synchronize()


def rc_of(dt, name, *args):
    from stfunet import _lib
    rc = getattr(_lib.load(dt), name)(*args, _lib.stream())
    torch.cuda.synchronize()
    return rc


def note(entry, ratio):
    WORST[entry] = max(WORST.get(entry, 0.0), ratio)
    print(f"{entry}: largest err / bound {ratio:.3f} (so far {WORST[entry]:.3f})")


def check16(entry, what, buf, ref, dt, kind, ab=None, k=0, skip=None):
    """The 16-bit output ``buf`` against the float64 ``ref``: equal to its rounding (exact run, or ab None),
    else within half a storage ulp + k 2^-23 ab; nothing outside the slice written."""
    assert buf.untouched_outside(), f"{what}: written outside its slice"
    got = buf.get()
    if kind == "exact" or ab is None:
        bad = got != ref.to(dt).double()
    else:
        assert not torch.isnan(got).any(), f"{what}: NaN (unwritten, or read outside an operand)"
        ratio = (got - ref).abs() / (R.half_ulp(ref, dt) + k * U23 * ab)
        if skip is not None:
            ratio = torch.where(skip, torch.zeros_like(ratio), ratio)
        note(entry, float(ratio.max()))
        bad = ratio > 1
    if skip is not None:
        assert float(skip.double().mean()) <= 1e-4, f"{what}: too many open mask decisions"
        bad = bad & ~skip
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements wrong, first at {i}: "
                             f"got {float(got[i])!r}, float64 {float(ref[i])!r}")


def check_sum(entry, what, got, ref, kind, bound=None):
    """fp32 sums against float64: equal (exact run), else within ``bound``."""
    if kind == "exact":
        bad = got != ref
    else:
        assert not torch.isnan(got).any(), f"{what}: NaN (an unwritten row, or a read outside an operand)"
        err = (got - ref).abs()
        note(entry, float((err / bound.clamp_min(1e-300)).max()))
        bad = err > bound
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} sums wrong, first at {i}: "
                             f"got {float(got[i])!r}, float64 {float(ref[i])!r}")


def vec(v):
    return R.F32(v, v.numel(), DEV)


def nanvec(n):
    return R.F32(None, n, DEV)


def intact(*bufs):
    for b in bufs:
        if b is not None:
            assert b.guards_intact(), "a sentinel word next to an fp32 buffer changed"


def p(b):
    return None if b is None else b.ptr


# ------------------------------------------------------------------ the entry points
def act_case(shape, kind, dt, res, relu, pooled=False, dev_gen=False):
    N, H, W, C, G = shape
    M, Mg, o = N * H * W, N * H * W // G, ops(shape, kind, dt, dev_gen)
    y, out = R.Slice16(o["y"], M, C, H * W, dt, DEV), R.Slice16(None, M, C, H * W, dt, DEV)
    sc, sh = vec(o["scale"]), vec(o["shift"])
    r = R.Slice16(o["res"], M, C, H * W, dt, DEV) if res else None
    rs, rh = (vec(o["rscale"]), vec(o["rshift"])) if res == 2 else (None, None)
    pl = R.Slice16(None, M // 4, C, H * W // 4, dt, DEV, wide=False) if pooled else None
    run(dt, "stf_bn_act", y.ptr, y.cs, N, H, W, C, G, sc.ptr, sh.ptr, relu, p(r), r.cs if r else 0, p(rs), p(rh),
        out.ptr, out.cs, p(pl))
    ref, ab, k = R.ref_act(o["y"], o["scale"], o["shift"], Mg, relu, o["res"] if res else None,
                           o["rscale"] if res == 2 else None, o["rshift"] if res == 2 else None)
    what = f"act {shape} res={res} relu={relu}"
    check16("stf_bn_act", what + " out", out, ref, dt, kind, ab, k)
    if pooled:
        check16("stf_bn_act", what + " pooled", pl, R.ref_pool2(R.rnd(ref, dt), shape)[0], dt, "exact")


def reduce_case(shape, kind, dt, mask, g_out, pooled=False, with_dz=True):
    from stfunet import _lib
    N, H, W, C, G = shape
    M, Mg, o = N * H * W, N * H * W // G, ops(shape, kind, dt)
    y = R.Slice16(o["y"], M, C, H * W, dt, DEV)
    dz = R.Slice16(o["dz"], M, C, H * W, dt, DEV) if with_dz else None
    dp = R.Slice16(o["dpool"], M // 4, C, H * W // 4, dt, DEV, wide=False) if pooled else None
    ms = R.Slice16(o["msrc"], M, C, H * W, dt, DEV) if mask == 2 else None
    sc, sh, mu, is_ = (vec(o[k]) for k in ("scale", "shift", "mean", "invstd"))
    go = R.Slice16(None, M, C, H * W, dt, DEV, wide=False) if g_out else None
    tpg = _lib.load(dt).stf_bn_bwd_tiles(N, H, W, C, G, int(pooled))
    part = nanvec(G * tpg * 2 * C)
    run(dt, "stf_bn_bwd_reduce", p(dz), dz.cs if dz else 0, p(dp), y.ptr, y.cs, N, H, W, C, G, sc.ptr, sh.ptr, mu.ptr,
        is_.ptr, mask, p(ms), ms.cs if ms else 0, p(go), part.ptr)
    d = o["dz"] if with_dz else torch.zeros_like(o["y"])
    if pooled:      # dpool goes to the window's first maximum of the rounded activation
        a = R.rnd(R.ref_act(o["y"], o["scale"], o["shift"], Mg, mask == 1)[0], dt)
        first = R.ref_pool2(a, shape)[1]
        dpx = R.unwindows2(o["dpool"].view(N, H // 2, W // 2, 1, C).expand(N, H // 2, W // 2, 4, C).contiguous(), shape)
        d = d + torch.where(first, dpx, torch.zeros_like(dpx))
    g, sums, bound, open_ = R.ref_reduce(d, o["y"], Mg, o["mean"], o["invstd"], mask, o["scale"], o["shift"],
                                         o["msrc"] if mask == 2 else None, kind == "exact")
    what = f"reduce {shape} mask={mask} g_out={g_out} pooled={pooled} dz={with_dz}"
    intact(part, sc, sh, mu, is_)
    if g_out:
        check16("stf_bn_bwd_reduce", what + " g_out", go, g, dt, kind, None, 0, open_ if kind == "gauss" else None)
    check_sum("stf_bn_bwd_reduce", what + " partial", part.get().view(G, tpg, 2, C).sum(1), sums, kind, bound)


def apply_case(shape, kind, dt, mask, bias, dev_gen=False):
    from stfunet import _lib
    N, H, W, C, G = shape
    M, Mg, o = N * H * W, N * H * W // G, ops(shape, kind, dt, dev_gen)
    g, y = R.Slice16(o["g"], M, C, H * W, dt, DEV), R.Slice16(o["y"], M, C, H * W, dt, DEV)
    dy, coef = R.Slice16(None, M, C, H * W, dt, DEV), vec(o["coef"])
    ms, mh = (vec(o["scale"]), vec(o["shift"])) if mask else (None, None)
    bp = nanvec(_lib.load(dt).stf_bn_bwd_apply_tiles(M, C) * C) if bias else None
    db = nanvec(C) if bias else None
    run(dt, "stf_bn_bwd_apply", g.ptr, g.cs, y.ptr, y.cs, M, C, G, p(ms), p(mh), coef.ptr, dy.ptr, dy.cs, p(bp), p(db))
    ref, ab, open_, dbias, dbound = R.ref_apply(o["g"], o["y"], o["coef"], Mg, o["scale"] if mask else None,
                                                o["shift"] if mask else None, kind == "exact")
    what = f"apply {shape} mask={mask} bias={bias}"
    intact(coef, ms, mh, bp, db)
    check16("stf_bn_bwd_apply", what + " dy", dy, ref, dt, kind, ab, 4, open_ if kind == "gauss" and mask else None)
    if bias:
        A = R.per_px(o["coef"][:, 0], Mg)
        dbound = dbound + torch.where(open_, (A * o["g"]).abs(), torch.zeros_like(A)).sum(0)   # open: in or out
        dkind = "gauss" if shape in R.DBIAS_BOUNDED else kind
        check_sum("stf_bn_bwd_apply", what + " dbias", db.get(), dbias, dkind, dbound)


OPT_ACT = [(r, a) for r in (0, 1, 2) for a in (0, 1)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", [s for s, _ in R.GROUP_MAJOR] + R.GENERIC, ids=_id)
def test_act(shape, dt, kind):
    for res, relu in OPT_ACT:
        act_case(shape, kind, dt, res, relu)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", [s for s, _ in R.GROUP_MAJOR], ids=_id)
def test_reduce(shape, dt, kind):
    for mask in (0, 1, 2):
        for g_out in (1, 0):
            reduce_case(shape, kind, dt, mask, g_out)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", [s for s, _ in R.GROUP_MAJOR], ids=_id)
def test_apply(shape, dt, kind):
    """dbias: the column sums of the fp32 dy BEFORE it is rounded to the storage type (the kernel's order)."""
    for mask in (0, 1):
        for bias in (0, 1):
            apply_case(shape, kind, dt, mask, bias)


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_act_and_plain_apply_past_the_block_cap(dt):
    """8.4 M units: the 8192-block grid makes a second, ragged grid-stride iteration.  Exact run, one option."""
    act_case(R.BIG, "exact", dt, 1, 1, dev_gen=True)
    torch.cuda.empty_cache()
    apply_case(R.BIG, "exact", dt, 1, 0, dev_gen=True)
    ops.cache_clear()


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", R.POOL_ACT, ids=_id)
def test_act_pool(shape, dt):
    for relu in (0, 1):
        act_case(shape, "exact", dt, 0, relu, pooled=True)


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", [s for s, _ in R.POOL_DPP + R.POOL_WIN], ids=_id)
def test_reduce_pool(shape, dt):
    for with_dz in (True, False):
        for mask in (0, 1):
            reduce_case(shape, "exact", dt, mask, 1, pooled=True, with_dz=with_dz)


# ------------------------------------------------------------------ the stem: MaxPool(3, 2, 1)
@pytest.mark.parametrize("codes", ["forward", "random"])
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", [s for s, _ in R.POOL3], ids=_id)
def test_pool3(shape, dt, codes):
    from stfunet import _lib
    N, H, W, C, G = shape
    M, Mg, o = N * H * W, N * H * W // G, ops(shape, "exact", dt)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Mo = N * Ho * Wo
    y = R.Slice16(o["y"], M, C, H * W, dt, DEV, wide=False)
    sc, sh, mu, is_, coef = (vec(o[k]) for k in ("scale", "shift", "mean", "invstd", "coef"))
    a = R.rnd(R.ref_act(o["y"], o["scale"], o["shift"], Mg, 1)[0], dt)
    out_ref, am_ref = R.ref_pool3_fwd(a, shape)
    if codes == "forward":          # stf_bn_act_maxpool3s2: out and argmax
        out = R.Slice16(None, Mo, C, Ho * Wo, dt, DEV, wide=False)
        amb = torch.full((3 * Mo, C), 0xEE, dtype=torch.uint8, device=DEV)
        run(dt, "stf_bn_act_maxpool3s2", y.ptr, N, H, W, C, G, sc.ptr, sh.ptr, out.ptr, amb[Mo:].data_ptr())
        check16("stf_bn_act_maxpool3s2", f"act_maxpool3s2 {shape} out", out, out_ref, dt, "exact")
        assert torch.equal(amb[Mo:2 * Mo], am_ref), f"act_maxpool3s2 {shape}: argmax is not the first maximum"
        assert bool((amb[:Mo] == 0xEE).all() and (amb[2 * Mo:] == 0xEE).all())
        am = am_ref
    else:
        am = o["argmax_rand"]
    amb = torch.full((3 * Mo, C), 0xEE, dtype=torch.uint8, device=DEV)      # 0xEE: no window position
    amb[Mo:2 * Mo] = am
    dout = R.Slice16(o["dout"], Mo, C, Ho * Wo, dt, DEV, wide=False)
    d = R.ref_pool3_bwd(am, o["dout"], shape, dt)
    g, sums, _, _ = R.ref_reduce(d, o["y"], Mg, o["mean"], o["invstd"], 1, o["scale"], o["shift"])
    tpg = _lib.load(dt).stf_bn_bwd_tiles(N, H, W, C, G, 0)
    part = nanvec(G * tpg * 2 * C)
    run(dt, "stf_bn_bwd_reduce_pool3", amb[Mo:].data_ptr(), dout.ptr, y.ptr, N, H, W, C, G, sc.ptr, sh.ptr, mu.ptr,
        is_.ptr, part.ptr)
    intact(part)
    check_sum("stf_bn_bwd_reduce_pool3", f"reduce_pool3 {shape} {codes}", part.get().view(G, tpg, 2, C).sum(1), sums,
              "exact")
    dy = R.Slice16(None, M, C, H * W, dt, DEV, wide=False)
    run(dt, "stf_bn_bwd_apply_pool3", amb[Mo:].data_ptr(), dout.ptr, y.ptr, N, H, W, C, G, sc.ptr, sh.ptr, coef.ptr,
        dy.ptr)
    check16("stf_bn_bwd_apply_pool3", f"apply_pool3 {shape} {codes}", dy, R.ref_apply(g, o["y"], o["coef"], Mg)[0], dt,
            "exact")


# ------------------------------------------------------------------ the finalizes
def ulp32(x, n=1):
    return n * U23 * x.abs()


def near(what, got, ref, bound, entry):
    assert not torch.isnan(got).any(), f"{what}: NaN"
    err = (got.view_as(ref) - ref).abs()
    note(entry, float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all()), f"{what}: off by {float((err / bound.clamp_min(1e-300)).max()):.3f} bounds"


def stat_rows(T, C, G, kind, seed):
    """[G][T][2][C] (sum, sum of squares) of 16 pixels per row: integers (any fold of them is exact), or
    Gaussian fp32.  Channel 0 is constant (variance 0) and channel 1's squares fall short of it (negative)."""
    gen = torch.Generator().manual_seed(seed)
    if kind == "exact":
        s = torch.stack([torch.randint(-50, 51, (G, T, C), generator=gen), torch.randint(200, 401, (G, T, C), generator=gen)], 2)
    else:
        s = torch.stack([torch.randn((G, T, C), generator=gen) * 10, torch.randn((G, T, C), generator=gen).abs() * 20 + 30], 2)
    s = s.float().double()
    s[:, :, 0, :2], s[:, :, 1, :2] = 48.0, 144.0
    s[:, 0, 1, 1] = 143.0
    return s.to(DEV)


FIN_CASES = [(c, k) for c in R.FINALIZE for k in KINDS if k == "exact" or c[0] <= R.ROW_CAP]


@pytest.mark.parametrize("mode", ["train", "train_norun", "eval", "eval_null"])
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("case,kind", FIN_CASES, ids=_id)
def test_finalize(case, kind, dt, mode):
    T, C, G = case
    Mtot = G * T * 16
    gen = torch.Generator().manual_seed(T * 7 + C)
    un = lambda lo, hi: (torch.rand(C, generator=gen) * (hi - lo) + lo).float().double().to(DEV)  # noqa: E731
    gamma, beta, rm0, rv0 = un(-1.5, 1.5), un(-0.5, 0.5), un(-0.5, 0.5), un(0.5, 2.0)
    train, running = mode.startswith("train"), mode in ("train", "eval")
    s = stat_rows(T, C, G, kind, T * 31 + C + G) if train else None
    stats = vec(s) if train else None
    rm, rv = (vec(rm0), vec(rv0)) if running else (None, None)
    outs = {k: nanvec(G * C) for k in ("mean", "invstd", "scale", "shift")}
    ga, be = vec(gamma), vec(beta)
    run(dt, "stf_bn_finalize", p(stats), T, G, C, Mtot, ga.ptr, be.ptr, R.MOM, R.EPS, p(rm), p(rv), outs["mean"].ptr,
        outs["invstd"].ptr, outs["scale"].ptr, outs["shift"].ptr)
    ref = R.ref_finalize(s, G, C, Mtot, gamma, beta, rm0 if running else None, rv0 if running else None)
    intact(stats, rm, rv, *outs.values())
    e, what = "stf_bn_finalize", f"finalize {case} {kind} {mode}"
    near(what + " mean", outs["mean"].get(), ref["mean"], ulp32(ref["mean"]), e)
    near(what + " invstd", outs["invstd"].get(), ref["invstd"], ulp32(ref["invstd"]), e)
    near(what + " scale", outs["scale"].get(), ref["scale"], ulp32(ref["scale"], 2), e)
    near(what + " shift", outs["shift"].get(), ref["shift"],
         2 * U23 * (beta.abs() + (ref["mean"] * ref["scale"]).abs()).expand(G, C), e)
    if train and running:
        near(what + " running_mean", rm.get(), ref["rm"], ref["rbound_m"], e)
        near(what + " running_var", rv.get(), ref["rv"], ref["rbound_v"], e)
    elif running:
        assert torch.equal(rm.get(), rm0) and torch.equal(rv.get(), rv0), "eval mode advanced the running statistics"
    if train:
        assert float(outs["invstd"].get().view(G, C)[:, :2].min()) > 300, "a zero / negative variance was not clamped"
    if train and G > 1:             # parked (mean, biased variance) in row 0 of every group
        parked = stats.get().view(G, T, 2, C)[:, 0]
        # the variance is a difference of two float64 terms, then one fp32 rounding
        vb = ulp32(ref["parked"][:, 1]) + 2.0 ** -48 * (ref["mean"] ** 2 + ref["parked"][:, 1])
        near(what + " parked mean", parked[:, 0], ref["parked"][:, 0], ulp32(ref["parked"][:, 0]), e)
        near(what + " parked var", parked[:, 1], ref["parked"][:, 1], vb, e)


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_finalize_one_pixel_per_group(dt):
    """Mg = 1: variance 0, and the running update takes the biased variance (no division by Mg - 1)."""
    C, G = 24, 3
    s = torch.stack([torch.arange(G * C, dtype=f64).view(G, 1, C) - 30, (torch.arange(G * C, dtype=f64).view(G, 1, C) - 30) ** 2],
                    2).to(DEV)
    one, zero = torch.ones(C, dtype=f64, device=DEV), torch.zeros(C, dtype=f64, device=DEV)
    stats, rm, rv, ga, be = vec(s), vec(zero), vec(one), vec(one), vec(zero)
    outs = {k: nanvec(G * C) for k in ("mean", "invstd", "scale", "shift")}
    run(dt, "stf_bn_finalize", stats.ptr, 1, G, C, G, ga.ptr, be.ptr, R.MOM, R.EPS, rm.ptr, rv.ptr, outs["mean"].ptr,
        outs["invstd"].ptr, outs["scale"].ptr, outs["shift"].ptr)
    ref = R.ref_finalize(s, G, C, G, one, zero, zero, one)
    intact(stats, rm, rv)
    e = "stf_bn_finalize"
    assert torch.equal(outs["mean"].get().view(G, C), ref["mean"])
    near("Mg=1 invstd", outs["invstd"].get(), ref["invstd"], ulp32(ref["invstd"]), e)
    near("Mg=1 running_var", rv.get(), ref["rv"], ref["rbound_v"], e)
    near("Mg=1 running_mean", rm.get(), ref["rm"], ref["rbound_m"], e)


@pytest.mark.parametrize("null", [0, 1])
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("case,kind", FIN_CASES, ids=_id)
def test_bwd_finalize(case, kind, dt, null):
    T, C, G = case
    Mtot = G * T * 16
    gen = torch.Generator().manual_seed(T * 13 + C + G)
    if kind == "exact":
        rows = torch.randint(-30, 31, (G, T, 2, C), generator=gen).double().to(DEV)
    else:
        rows = torch.randn((G, T, 2, C), generator=gen).float().double().to(DEV)
    un = lambda lo, hi, *s: (torch.rand(s, generator=gen) * (hi - lo) + lo).float().double().to(DEV)  # noqa: E731
    gamma, mean, invstd = un(-1.5, 1.5, C), un(-0.5, 0.5, G, C), un(0.5, 2.0, G, C)
    part, ga, mu, is_ = vec(rows), vec(gamma), vec(mean), vec(invstd)
    dg, db = (None, None) if null else (nanvec(C), nanvec(C))
    coef = nanvec(G * 3 * C)
    run(dt, "stf_bn_bwd_finalize", part.ptr, T, G, C, Mtot, ga.ptr, mu.ptr, is_.ptr, p(dg), p(db), coef.ptr)
    sums = rows.sum(1)
    ref = R.ref_bwd_finalize(sums, G, C, Mtot, gamma, mean, invstd)
    intact(part, coef, dg, db)
    e, what = "stf_bn_bwd_finalize", f"bwd_finalize {case} {kind} null={null}"
    cb = torch.stack([ref["coef"][:, 0].abs(), ref["coef"][:, 1].abs(), ref["cabs"]], 1) * U23
    near(what + " coef", coef.get(), ref["coef"], cb, e)
    sbound = (G + 1) * U23 * sums.abs().sum(0)
    if not null:
        check_sum(e, what + " dgamma", dg.get(), ref["dgamma"], kind, sbound[1])
        check_sum(e, what + " dbeta", db.get(), ref["dbeta"], kind, sbound[0])
    elif G > 1:                     # nothing summed: each group's (sum g, sum g*xhat) stays parked in its row 0
        parked = part.get().view(G, T, 2, C)[:, 0]
        check_sum(e, what + " parked", parked, sums, kind, U23 * sums.abs())


# ------------------------------------------------------------------ the batched tails
class RunDesc(ctypes.Structure):
    _fields_ = [("stats", ctypes.c_void_p), ("running_mean", ctypes.c_void_p), ("running_var", ctypes.c_void_p),
                ("Mg", ctypes.c_int64), ("tiles", ctypes.c_int), ("groups", ctypes.c_int), ("C", ctypes.c_int),
                ("momentum", ctypes.c_float)]


class GsumDesc(ctypes.Structure):
    _fields_ = [("partial", ctypes.c_void_p), ("dgamma", ctypes.c_void_p), ("dbeta", ctypes.c_void_p),
                ("tiles", ctypes.c_int), ("groups", ctypes.c_int), ("C", ctypes.c_int)]


def batch_items(count):
    return [((8, 24, 64, 2048)[i % 4], 2 + i % 3, 1 + i % 4) for i in range(count)]        # (C, groups, tiles)


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("count", R.BATCH_COUNTS)
def test_running_batch(count, dt):
    """More than one 32-descriptor chunk: bit for bit the in-call update, and within the reference's bound."""
    keep, descs, want = [], [], []
    for i, (C, G, T) in enumerate(batch_items(count)):
        s = stat_rows(T, C, G, "gauss", 1000 + i)
        Mtot = G * T * 16
        gen = torch.Generator().manual_seed(i)
        un = lambda lo, hi: (torch.rand(C, generator=gen) * (hi - lo) + lo).float().double().to(DEV)  # noqa: E731
        gamma, beta, rm0, rv0 = un(-1.5, 1.5), un(-0.5, 0.5), un(-0.5, 0.5), un(0.5, 2.0)
        ga, be = vec(gamma), vec(beta)
        res = []
        for deferred in (False, True):
            stats, rm, rv = vec(s), vec(rm0), vec(rv0)
            outs = [nanvec(G * C) for _ in range(4)]
            run(dt, "stf_bn_finalize", stats.ptr, T, G, C, Mtot, ga.ptr, be.ptr, R.MOM, R.EPS, None if deferred else rm.ptr,
                None if deferred else rv.ptr, *[o.ptr for o in outs])
            res.append((stats, rm, rv))
        descs.append(RunDesc(res[1][0].ptr, res[1][1].ptr, res[1][2].ptr, Mtot // G, T, G, C, R.MOM))
        keep.append(res)
        want.append(R.ref_finalize(s, G, C, Mtot, gamma, beta, rm0, rv0))
    arr = (RunDesc * count)(*descs)
    run(dt, "stf_bn_running_batch", arr, count)
    for i, (res, ref) in enumerate(zip(keep, want)):
        (_, rm_in, rv_in), (st, rm, rv) = res
        intact(st, rm, rv)
        assert torch.equal(rm.get(), rm_in.get()) and torch.equal(rv.get(), rv_in.get()), f"descriptor {i}"
        near(f"running_batch {i} mean", rm.get(), ref["rm"], ref["rbound_m"], "stf_bn_running_batch")
        near(f"running_batch {i} var", rv.get(), ref["rv"], ref["rbound_v"], "stf_bn_running_batch")


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("count", R.BATCH_COUNTS)
def test_groupsum_batch(count, dt):
    keep, descs = [], []
    for i, (C, G, T) in enumerate(batch_items(count)):
        gen = torch.Generator().manual_seed(2000 + i)
        rows = torch.randint(-30, 31, (G, T, 2, C), generator=gen).double().to(DEV)
        ones = torch.ones(G, C, dtype=f64, device=DEV)
        ga, mu, is_ = vec(ones[0]), vec(ones), vec(ones)
        res = []
        for deferred in (False, True):
            part, dg, db, coef = vec(rows), nanvec(C), nanvec(C), nanvec(G * 3 * C)
            run(dt, "stf_bn_bwd_finalize", part.ptr, T, G, C, G * T * 16, ga.ptr, mu.ptr, is_.ptr, None if deferred else dg.ptr,
                None if deferred else db.ptr, coef.ptr)
            res.append((part, dg, db))
        descs.append(GsumDesc(res[1][0].ptr, res[1][1].ptr, res[1][2].ptr, T, G, C))
        keep.append((res, rows.sum(1).sum(0)))
    arr = (GsumDesc * count)(*descs)
    run(dt, "stf_bn_groupsum_batch", arr, count)
    for i, (res, tot) in enumerate(keep):
        (_, dg_in, db_in), (part, dg, db) = res
        intact(part, dg, db)
        assert torch.equal(dg.get(), dg_in.get()) and torch.equal(db.get(), db_in.get()), f"descriptor {i}"
        assert torch.equal(db.get(), tot[0]) and torch.equal(dg.get(), tot[1]), f"descriptor {i}: not the exact sum"


# ------------------------------------------------------------------ argument checks
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_einval_writes_nothing(dt):
    """Every documented STF_EINVAL of these entry points returns it and launches nothing: outputs stay NaN."""
    shape = N, H, W, C, G = (2, 4, 4, 16, 2)
    M, o = N * H * W, ops(shape, "exact", dt)
    S = lambda name, rows=M, wide=True: R.Slice16(o[name], rows, C, rows // N, dt, DEV, wide)  # noqa: E731
    y, dz, res, ms, dp = S("y"), S("dz"), S("res"), S("msrc"), S("dpool", M // 4, False)
    out, pl, go = R.Slice16(None, M, C, H * W, dt, DEV), R.Slice16(None, M // 4, C, H * W // 4, dt, DEV, False), \
        R.Slice16(None, M, C, H * W, dt, DEV, False)
    sc, sh, mu, is_, coef = (vec(o[k]) for k in ("scale", "shift", "mean", "invstd", "coef"))
    part, fo = nanvec(4096), [nanvec(G * C) for _ in range(4)]
    am = torch.zeros((M, C), dtype=torch.uint8, device=DEV)
    E = R.EINVAL

    def act(N=N, H=H, C=C, G=G, ycs=y.cs, ocs=out.cs, res=None, rcs=0, pooled=None):
        return rc_of(dt, "stf_bn_act", y.ptr, ycs, N, H, W, C, G, sc.ptr, sh.ptr, 1, res, rcs, None, None, out.ptr, ocs, pooled)
    assert [act(C=12), act(ycs=y.cs + 4), act(ocs=out.cs + 4), act(H=3, pooled=pl.ptr), act(G=0), act(N=3),
            act(res=res.ptr, rcs=res.cs + 4), act(res=res.ptr, rcs=res.cs, pooled=pl.ptr)] == [E] * 8

    def red(C=C, N=N, H=H, G=G, ycs=y.cs, dzp=dz.ptr, dzcs=dz.cs, dpool=None, mask=1, msrc=None, mcs=0, g_out=go.ptr):
        return rc_of(dt, "stf_bn_bwd_reduce", dzp, dzcs, dpool, y.ptr, ycs, N, H, W, C, G, sc.ptr, sh.ptr, mu.ptr, is_.ptr,
                     mask, msrc, mcs, g_out, part.ptr)
    assert [red(C=24), red(ycs=y.cs + 4), red(dzcs=dz.cs + 4), red(G=0), red(N=3), red(dzp=None), red(dpool=dp.ptr, g_out=None),
            red(dpool=dp.ptr, H=3), red(dpool=dp.ptr, mask=2, msrc=ms.ptr, mcs=ms.cs), red(mask=2), red(mask=2, msrc=ms.ptr, mcs=ms.cs + 4)] \
        == [E] * 11

    def app(C=C, M=M, G=G, gcs=dz.cs, ycs=y.cs, dcs=out.cs, msc=None, msh=None):
        return rc_of(dt, "stf_bn_bwd_apply", dz.ptr, gcs, y.ptr, ycs, M, C, G, msc, msh, coef.ptr, out.ptr, dcs, None, None)
    assert [app(C=24), app(gcs=dz.cs + 4), app(ycs=y.cs + 4), app(dcs=out.cs + 4), app(G=0), app(M=M + 1), app(msc=sc.ptr),
            app(msh=sh.ptr)] == [E] * 8

    def fin(name, G, Mtot):
        if name == "stf_bn_finalize":
            return rc_of(dt, name, None, 1, G, C, Mtot, sc.ptr, sh.ptr, R.MOM, R.EPS, None, None, *[f.ptr for f in fo])
        return rc_of(dt, name, part.ptr, 1, G, C, Mtot, sc.ptr, mu.ptr, is_.ptr, None, None, fo[0].ptr)
    assert [fin(n, g, m) for n in ("stf_bn_finalize", "stf_bn_bwd_finalize") for g, m in ((0, 8), (3, 8))] == [E] * 4

    yd, dod = S("y", M, False), S("dz", M, False)      # dense, as the pool3 entry points take them

    def p3(name, a=am.data_ptr(), d=dod.ptr, yy=yd.ptr, N=N, C=C, G=G, last=None):
        tail = (sc.ptr, sh.ptr, mu.ptr, is_.ptr, part.ptr if last is None else last[0]) if name.endswith("reduce_pool3") \
            else (sc.ptr, sh.ptr, coef.ptr, go.ptr if last is None else last[0])
        return rc_of(dt, name, a, d, yy, N, H, W, C, G, *tail)
    for name in ("stf_bn_bwd_reduce_pool3", "stf_bn_bwd_apply_pool3"):
        assert [p3(name, a=None), p3(name, d=None), p3(name, yy=None), p3(name, last=(None,)), p3(name, G=0), p3(name, N=3),
                p3(name, C=24)] == [E] * 7

    def ap3(yy=yd.ptr, C=C, G=G, N=N, s=sc.ptr, h=sh.ptr, o_=go.ptr):
        return rc_of(dt, "stf_bn_act_maxpool3s2", yy, N, H, W, C, G, s, h, o_, am.data_ptr())
    assert [ap3(yy=None), ap3(C=12), ap3(G=0), ap3(N=3), ap3(s=None), ap3(h=None), ap3(o_=None)] == [E] * 7

    rd = lambda **k: (RunDesc * 1)(RunDesc(**{**dict(stats=part.ptr, running_mean=fo[0].ptr, running_var=fo[1].ptr, Mg=4, tiles=1,  # noqa: E731
                                                    groups=2, C=C, momentum=R.MOM), **k}))
    assert [rc_of(dt, "stf_bn_running_batch", rd(**k), 1) for k in (dict(stats=None), dict(running_mean=None), dict(running_var=None),
                                                                     dict(groups=0), dict(C=0), dict(tiles=0))] == [E] * 6
    gd = lambda **k: (GsumDesc * 1)(GsumDesc(**{**dict(partial=part.ptr, dgamma=fo[0].ptr, dbeta=fo[1].ptr, tiles=1, groups=2, C=C),  # noqa: E731
                                                 **k}))
    assert [rc_of(dt, "stf_bn_groupsum_batch", gd(**k), 1) for k in (dict(partial=None), dict(groups=0), dict(C=0), dict(tiles=0))] \
        == [E] * 4
    # nothing was launched: every output is still NaN, every sentinel in place
    for b in (out, pl, go):
        assert bool(torch.isnan(b.buf).all())
    for b in [part] + fo:
        assert bool(torch.isnan(b.get()).all())
    intact(part, *fo)
