"""The head at 1 to 4 classes (csrc/head.hip) and the streaming tail kernels of csrc/stf.hip / csrc/misc.hip
against float64, per element, through the C entry points only.

The cases, operands and references are tests/_tail_ref.py's (tests/test_tail_parity_cpu.py checks them without a
GPU).  Every kernel has two legs.  Exact: integer / dyadic operands, every fp32 intermediate exact in any order, so
every output must EQUAL float64 (per-tile partials are added in float64 on the host).  Gaussian: an output stays
within gamma(n + c) * sum |terms| (n terms, c fp32 roundings behind a term, gamma(m) = m u / (1 - m u), u = 2^-24),
plus half a storage ulp of the reference for a 16-bit output; an element whose ReLU decision lies within the fp32
slack of zero is left out (at most 1e-4 of a case) and its worst case is added to the bound of the sums it enters.
Each Gaussian comparison prints its largest err / bound.

Buffers: outputs start as NaN and must be finite afterwards; 16-bit tensors have a NaN image before and after (and
NaN channels beside them where the entry point takes a stride), fp32 buffers sit between sentinel words; two runs of
the head give the same bits.
"""
import functools

import pytest
import torch

import _tail_ref as T
from _tail_ref import F32, Slice16, gamma, half_ulp

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
KINDS = ["exact", "gauss"]
WORST = {}                               # entry point -> largest err / bound of the Gaussian legs so far
f64 = torch.float64


def _id(v):
    return "bf16" if v is torch.bfloat16 else "fp16" if v is torch.float16 else str(v).replace(" ", "")


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


def run(dt, name, *args):
    from stfunet import _lib
    with _lib.storage(dt):
        _lib.call(name, *args, _lib.stream())
    torch.cuda.synchronize()


def note(entry, ratio):
    WORST[entry] = max(WORST.get(entry, 0.0), ratio)
    print(f"{entry}: largest err / bound {ratio:.3f} (so far {WORST[entry]:.3f})")


def compare(entry, what, got, ref, bound=None, skip=None):
    """``got`` against the float64 ``ref``: equal (bound None), else within ``bound``; ``skip``: elements left out."""
    got = got.reshape(ref.shape)
    lost = ~torch.isfinite(got)
    if bool(lost.any()):
        i = tuple(int(v) for v in lost.nonzero()[0])
        raise AssertionError(f"{what}: {int(lost.sum())} of {lost.numel()} elements not finite (unwritten, or read from "
                             f"outside an operand), first at {i}")
    if bound is None:
        bad = got != ref
    else:
        ratio = (got - ref).abs() / bound.clamp_min(1e-300)
        if skip is not None:
            ratio = torch.where(skip, torch.zeros_like(ratio), ratio)
        note(entry, float(ratio.max()))
        bad = ratio > 1
    if skip is not None:
        assert float(skip.double().mean()) <= 1e-4, f"{what}: too many open ReLU decisions"
        bad = bad & ~skip
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements wrong, first at {i}: "
                             f"got {float(got[i])!r}, float64 {float(ref[i])!r}")


def vec(v):
    return F32(v.to(DEV), v.numel(), DEV)


def nanvec(n):
    return F32(None, n, DEV)


def intact(*bufs):
    for b in bufs:
        if isinstance(b, Slice16):
            assert b.untouched_outside(), "written outside a 16-bit slice"
        else:
            assert b.guards_intact(), "a sentinel word next to an fp32 buffer changed"


# ------------------------------------------------------------------ head, 1 to 4 classes
def head_case(shape, C, K, kind, dt, identity, families):
    from stfunet import _lib
    N, H, W = shape
    P = N * H * W
    o = T.HeadOps(shape, C, K, kind, dt, identity).to(DEV)
    ref = T.head_ref(o, bounds=kind == "gauss")
    y = Slice16(o.y, P, C, H * W, dt, DEV, wide=False)
    sc, sh, mu, is_, w, b, dl = (vec(getattr(o, n)) for n in ("scale", "shift", "mean", "invstd", "w", "bias", "dl"))
    tiles = _lib.load(dt).stf_head_tiles(N, H, W, C)
    assert tiles == T.head_tiles(P, C)
    bd = (lambda k: ref["b_" + k]) if kind == "gauss" else (lambda k: None)
    for fam in families:
        bits = []
        for _ in range(2):
            logits, dw, db = nanvec(N * K * H * W), nanvec(K * C), nanvec(K)
            g = Slice16(None, P, C, H * W, dt, DEV, wide=False)
            bnp, hp = nanvec(tiles * 2 * C), nanvec((tiles + 1) * K * (C + 1))
            run(dt, fam + "_fwd", y.ptr, N, H, W, C, sc.ptr, sh.ptr, w.ptr, b.ptr, K, logits.ptr)
            run(dt, fam + "_bwd", dl.ptr, y.ptr, N, H, W, C, sc.ptr, sh.ptr, mu.ptr, is_.ptr, w.ptr, K, g.ptr, bnp.ptr,
                hp.ptr, dw.ptr, db.ptr)
            bits.append([logits.mid.view(torch.int32).clone(), g.buf.view(torch.int16).clone(),
                         bnp.mid.view(torch.int32).clone(), dw.mid.view(torch.int32).clone(), db.mid.view(torch.int32).clone()])
        what = f"{fam} {shape} C={C} K={K} {kind} {_id(dt)} identity={identity}"
        compare(fam + "_fwd", what + " logits", logits.get(), ref["logits"], bd("logits"))
        assert logits.guards_intact(), what + ": a logit was written outside [N][K][H][W]"
        intact(dw, db, bnp, hp, g, y, sc, sh, mu, is_, w, b, dl)
        gb = None if kind == "exact" else ref["b_g"] + half_ulp(ref["g"], dt)
        compare(fam + "_bwd g", what + " g", g.get(), ref["g"], gb, ref.get("open"))
        compare(fam + "_bwd dW", what + " dW", dw.get(), ref["dW"], bd("dW"))
        compare(fam + "_bwd db", what + " db", db.get(), ref["db"], bd("db"))
        # every one of the ``tiles`` rows is read by the consumer: all finite, their float64 sum the reference's
        compare(fam + "_bwd bn_partial", what + " bn_partial", bnp.get().view(tiles, 2, C).sum(0), ref["sums"], bd("sums"))
        assert bool(torch.isfinite(bnp.get()).all()), what + ": a bn_partial row was left unwritten"
        for a, c, name in zip(bits[0], bits[1], ("logits", "g", "bn_partial", "dW", "db")):
            assert torch.equal(a, c), f"{what}: {name} differs between two runs"


def families(kind):
    """The many-class kernels take 1 to 4 classes too: the exact run pins both families to the same reference."""
    return ("stf_head", "stf_head_mc") if kind == "exact" else ("stf_head",)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("C", T.HEAD_C)
@pytest.mark.parametrize("shape", T.HEAD_GRID, ids=_id)
def test_head(shape, C, dt, kind):
    for K in T.HEAD_K:
        for identity in (False, True):
            head_case(shape, C, K, kind, dt, identity, families(kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", T.HEAD_C)
def test_head_one_pixel(C, kind):
    shape, K, dt = T.HEAD_PIXEL
    head_case(shape, C, K, kind, T.DTYPES[dt], False, families(kind))


def test_head_past_the_forward_block_cap():
    """3.1 M units: the forward's 8192 blocks take a second, half-filled round of their four (and two empty ones), the
    backward's 1024 tiles make twelve grid-stride passes.  Exact run."""
    shape, C, K, dt = T.HEAD_CAP
    head_case(shape, C, K, "exact", T.DTYPES[dt], False, families("exact"))


# ------------------------------------------------------------------ MaxPool(3, 2, 1)
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("C", T.POOL_C)
@pytest.mark.parametrize("hw", T.POOL_HW, ids=_id)
def test_maxpool3(hw, C, dt):
    """Ties and negative windows (the -inf start needs no ReLU'd input): forward and argmax are F.max_pool2d's, the
    backward its float64 scatter."""
    (H, W), N = hw, T.POOL_N
    Ho, Wo = T.pool_out(H), T.pool_out(W)
    M, Mo = N * H * W, N * Ho * Wo
    x = T.pool_input(H, W, C)
    gen = T._gen("pool_d", hw, C, str(dt))
    d_int = T.ri(gen, -8, 8, N, C, Ho, Wo)
    d_gauss = torch.randn((N, C, Ho, Wo), generator=gen).to(dt).double()
    out_ref, codes, dx_int, _ = T.pool_ref(x, d_int)
    _, _, dx_gauss, ab = T.pool_ref(x, d_gauss)
    xs = Slice16(T.nhwc(x).to(DEV), M, C, H * W, dt, DEV, wide=False)
    out = Slice16(None, Mo, C, Ho * Wo, dt, DEV, wide=False)
    amb = torch.full((3 * Mo, C), 0xEE, dtype=torch.uint8, device=DEV)
    run(dt, "stf_maxpool3s2_fwd", xs.ptr, N, H, W, C, out.ptr, amb[Mo:].data_ptr())
    what = f"maxpool3 {hw} C={C} {_id(dt)}"
    intact(xs, out)
    compare("stf_maxpool3s2_fwd", what + " out", out.get(), T.nhwc(out_ref).to(DEV))
    bad = amb[Mo:2 * Mo] != T.nhwc(codes).to(DEV)
    assert not bool(bad.any()), f"{what}: argmax is not torch's index, first at {tuple(int(v) for v in bad.nonzero()[0])}"
    assert bool((amb[:Mo] == 0xEE).all() and (amb[2 * Mo:] == 0xEE).all()), what + ": argmax written outside"
    for d, ref, bound in ((d_int, dx_int, None), (d_gauss, dx_gauss, gamma(5) * ab)):
        ds = Slice16(T.nhwc(d).to(DEV), Mo, C, Ho * Wo, dt, DEV, wide=False)
        dx = Slice16(None, M, C, H * W, dt, DEV, wide=False)
        run(dt, "stf_maxpool3s2_bwd", amb[Mo:].data_ptr(), ds.ptr, N, H, W, C, dx.ptr)
        intact(ds, dx)
        r = T.nhwc(ref).to(DEV)
        compare("stf_maxpool3s2_bwd", what + " dx", dx.get(), r, None if bound is None else T.nhwc(bound).to(DEV) + half_ulp(r, dt))


# ------------------------------------------------------------------ bilinear, align_corners=True
def resize_kinds(shape):
    return KINDS if shape in T.RESIZE_DYADIC else ["gauss"]


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("C", T.RESIZE_C)
@pytest.mark.parametrize("shape", T.RESIZE, ids=_id)
def test_bilinear_ac(shape, C, dt):
    """Channel slices of wider NaN buffers on both sides.  The backward reference scatters the forward's own tables:
    it knows nothing of the kernel's candidate window."""
    (H, W, h, w), N = shape, T.RESIZE_N
    for kind in resize_kinds(shape):
        x = T.resize_input(shape, kind, dt, "x", N, H, W, C).to(DEV)
        dy = T.resize_input(shape, kind, dt, "dy", N, h, w, C).to(DEV)
        xs, ys = Slice16(x.view(-1, C), N * H * W, C, H * W, dt, DEV), Slice16(None, N * h * w, C, h * w, dt, DEV)
        run(dt, "stf_bilinear_ac_fwd", xs.ptr, N, H, W, C, xs.cs, ys.ptr, h, w, ys.cs)
        ref, ab = T.resize_fwd(x, h, w)
        what = f"bilinear_ac {shape} C={C} {kind} {_id(dt)}"
        intact(xs, ys)
        compare("stf_bilinear_ac_fwd", what + " y", ys.get(), ref,
                None if kind == "exact" else gamma(7) * ab + half_ulp(ref, dt))
        dys, dxs = Slice16(dy.view(-1, C), N * h * w, C, h * w, dt, DEV), Slice16(None, N * H * W, C, H * W, dt, DEV)
        run(dt, "stf_bilinear_ac_bwd", dys.ptr, N, h, w, C, dys.cs, dxs.ptr, H, W, dxs.cs)
        ref, ab, cnt = T.resize_bwd(dy, H, W)
        intact(dys, dxs)
        # a term: wy and wx (an add each where both taps are the pixel), their product, the product with dy
        compare("stf_bilinear_ac_bwd", what + " dx", dxs.get(), ref,
                None if kind == "exact" else gamma(cnt + 4).view(1, H, W, 1) * ab + half_ulp(ref, dt))


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("P", [1, 3, 8])
@pytest.mark.parametrize("shape", T.RESIZE, ids=_id)
def test_bilinear_ac_bwd_tsum(shape, P, dt):
    """The PK maps' input gradient: ADDED into frames T .. T+P-1 of a prefilled [B][Ttot][H][W] fp32 tensor through its
    own batch / channel strides; every other frame keeps its value."""
    (H, W, h, w), Tn, B = shape, 3, 2
    Ttot = Tn + 8
    for kind in resize_kinds(shape):
        dy = T.resize_input(shape, kind, dt, "tsum", Tn * B, h, w, 8).to(DEV)
        dys = Slice16(dy.view(-1, 8), Tn * B * h * w, 8, h * w, dt, DEV)
        pre = T.ri(T._gen("tsum_pre", shape), -8, 8, B, Ttot, H, W).to(DEV)
        out = vec(pre)
        run(dt, "stf_bilinear_ac_bwd_tsum", dys.ptr, Tn, B, h, w, dys.cs, P, out.ptr + 4 * Tn * H * W, Ttot * H * W, H * W, H, W)
        frames = dy.view(Tn, B, h, w, 8)
        dx, _, cnt = T.resize_bwd(frames.sum(0), H, W)
        ab = T.resize_bwd(frames.abs().sum(0), H, W)[1]
        want, bound = pre.clone(), torch.zeros_like(pre)
        want[:, Tn:Tn + P] += dx[..., :P].permute(0, 3, 1, 2)
        # a term: Tn - 1 adds, wy, wx, their product, the product with the sum; then the add into the prefilled value
        bound[:, Tn:Tn + P] = (gamma(cnt + Tn + 5).view(1, H, W, 1) * (ab + pre[:, Tn:].permute(0, 2, 3, 1).abs())
                               )[..., :P].permute(0, 3, 1, 2)
        intact(dys, out)
        compare("stf_bilinear_ac_bwd_tsum", f"bwd_tsum {shape} P={P} {kind} {_id(dt)}", out.get(), want,
                None if kind == "exact" else bound)


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("shape", T.RESIZE, ids=_id)
def test_pk_resize(shape, P, dt):
    """fp32 maps [B][Ttot][H][W] (frames T .. T+P-1) resized into channels coff .. coff+P-1 of every time step's rows."""
    (H, W, h, w), Tn, B = shape, 2, 2
    Ttot = Tn + P + 1
    for kind in resize_kinds(shape):
        x = T.resize_input(shape, kind, None, "pk", B, Ttot, H, W).to(DEV)
        xb = vec(x)
        dst = Slice16(None, Tn * B * h * w, P, h * w, dt, DEV)
        rows = dst.buf[dst.img:]
        run(dt, "stf_pk_resize", xb.ptr, B, Ttot, Tn, P, H, W, h, w, rows.data_ptr(), dst.cs, dst.off)
        ref, ab = T.resize_fwd(x[:, Tn:Tn + P].permute(0, 2, 3, 1).contiguous(), h, w)
        ref, ab = ref.repeat(Tn, 1, 1, 1).view(-1, P), ab.repeat(Tn, 1, 1, 1).view(-1, P)
        intact(xb, dst)
        compare("stf_pk_resize", f"pk_resize {shape} P={P} {kind} {_id(dt)}", dst.get(), ref,
                None if kind == "exact" else gamma(7) * ab + half_ulp(ref, dt))


# ------------------------------------------------------------------ packs: pure roundings
def check_pack(what, out, want, C):
    got = out.buf[out.img:out.img + out.M].cpu()
    assert out.untouched_outside(), what + ": written outside"
    assert bool((got[:, C:].view(torch.int16) == 0).all()), what + ": a padding channel is not +0"
    if not T.same16(got, want):
        bad = ((got.view(torch.int16) != want.view(torch.int16)) & ~(torch.isnan(got) & torch.isnan(want))).nonzero()[0]
        i = tuple(int(v) for v in bad)
        raise AssertionError(f"{what}: not torch's rounding at {i}: got bits {int(got.view(torch.int16)[i]) & 0xFFFF:#06x}, "
                             f"torch {int(want.view(torch.int16)[i]) & 0xFFFF:#06x}")


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("cc", T.PACK_C, ids=_id)
def test_pack_input(cc, dt):
    (C, Cpad), N, H, W = cc, 2, 17, 23
    x = T.pack_values(dt, N * C * H * W, ("input", C)).view(N, C, H, W)
    xb = x.to(DEV)
    out = Slice16(None, N * H * W, Cpad, H * W, dt, DEV, wide=False)
    run(dt, "stf_pack_input", xb.data_ptr(), N, C, H, W, Cpad, out.ptr)
    check_pack(f"pack_input C={C} Cpad={Cpad} {_id(dt)}", out, T.pack_input_ref(x, Cpad, dt), C)


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("ccp", [(C, Cpad, 0) for C, Cpad in T.PACK_C] + [(1, 8, 3)], ids=_id)
def test_pack_sequence(ccp, dt):
    (C, Cpad, P), B, Tn, H, W = ccp, 2, 3, 9, 13
    Ttot = Tn + P + 1
    x = T.pack_values(dt, B * Ttot * C * H * W, ("sequence", C, P)).view(B, Ttot, C, H, W)
    xb = x.to(DEV)
    out = Slice16(None, Tn * B * H * W, Cpad, H * W, dt, DEV, wide=False)
    run(dt, "stf_pack_sequence", xb.data_ptr(), B, Ttot, C, H, W, Tn, P, Cpad, out.ptr)
    check_pack(f"pack_sequence C={C} Cpad={Cpad} P={P} {_id(dt)}", out, T.pack_sequence_ref(x, Tn, P, Cpad, dt), C + P)


# ------------------------------------------------------------------ channel_sum / stat_sums: exact on integers
@functools.lru_cache(maxsize=1)
def csum_input(M, C):
    return T.ri(T._gen("csum", M, C), -8, 8, M, C).to(DEV)


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("C", T.CSUM_C)
@pytest.mark.parametrize("M", T.CSUM_M)
def test_channel_sum(M, C, dt):
    x = csum_input(M, C)
    xs = Slice16(x, M, C, min(M, 64), dt, DEV)
    tiles = T.csum_tiles(M, C)
    part, out = nanvec(tiles * C), nanvec(C)
    run(dt, "stf_channel_sum", xs.ptr, xs.cs, M, C, part.ptr, out.ptr)
    intact(xs, part, out)
    compare("stf_channel_sum", f"channel_sum M={M} C={C} {_id(dt)}", out.get(), x.sum(0))


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("cols", T.STAT_COLS, ids=_id)
@pytest.mark.parametrize("tiles", T.STAT_TILES)
def test_stat_sums(tiles, cols, dt):
    """Columns c0 .. c0+C-1 of the sum half of [tiles][2][Nout]; the squares half holds a value that would show."""
    Nout, c0, C = cols
    s = T.ri(T._gen("stat", tiles, cols), -50, 50, tiles, 2, Nout)
    s[:, 1] = 2.0 ** 20
    stats, out = vec(s), nanvec(C)
    run(dt, "stf_stat_sums", stats.ptr, tiles, Nout, c0, C, out.ptr)
    intact(stats, out)
    compare("stf_stat_sums", f"stat_sums tiles={tiles} {cols}", out.get(), s[:, 0, c0:c0 + C].sum(0).to(DEV))
