"""Every implicit-GEMM variant an unforced launch can select, against a float64 restatement.

The cases are tests/_igemm_variants.py's table (tests/test_igemm_variants_cpu.py checks that it names
every reachable variant) in both storage types.  Each case builds operands already rounded to the
storage type, pre-fills the destination buffer with NaN (a random base where the launch accumulates),
asserts the kernel name the router gives for the actual arguments, launches once and compares with
float64 conv2d / conv_transpose2d / autograd of conv2d (on the device where torch has the op in
float64, else on the CPU) or, for the LSTM epilogues, a float64 restatement of oracle/stf.py's cell.

Bounds are the project's (test_kernels_gpu.py, test_fp16_gpu.py): relative L2 of 16-bit outputs
1e-2 (bf16) / 2e-3 (fp16), of fp32 BN statistics 2e-3 / 1e-3, fused BN-backward partials 1e-5 -- applied
per image (statistics: per group) and per 64-channel slice, so a dropped or misplaced tile cannot hide
in a whole-tensor norm.  Channels of the destination buffer outside the written slice must keep their
NaN bits.  The last tests run sources, destinations and a fused BN-backward y of 4.5 GiB.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _igemm_variants as V

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
BOUND_16 = {torch.bfloat16: 1e-2, torch.float16: 2e-3}        # 16-bit outputs
BOUND_STATS = {torch.bfloat16: 2e-3, torch.float16: 1e-3}     # fp32 BN partial statistics
BOUND_BNR = 1e-5                                              # fused BN-backward partials
# LSTM epilogue outputs: twice lstm_emulation_error() (see test_lstm_bounds_are_twice_the_emulation_error)
BOUND_LSTM = {
    torch.bfloat16: {"gates": 2.66e-3, "c_out": 2.82e-3, "h_out": 4.76e-3, "dgates": 5.45e-3, "dc_prev": 2.14e-3},
    torch.float16: {"gates": 3.26e-4, "c_out": 3.42e-4, "h_out": 5.96e-4, "dgates": 6.60e-4, "dc_prev": 2.69e-4}}
MARGIN = 8                                                    # channels each side of a slice of a 4.5 GiB buffer


def _id(v):
    return "bf16" if v is torch.bfloat16 else "fp16" if v is torch.float16 else None


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(0)
    yield
    torch.cuda.empty_cache()


def f64(fn):
    """fn(device) in float64 on the GPU where torch has the ops there, else on the CPU; result on the GPU."""
    try:
        return fn(DEV).to(DEV)
    except RuntimeError:
        return fn("cpu").to(DEV)


def worst_rel(out, ref, rows):
    """Largest relative L2 error over (image or group, 64-channel slice) blocks of [rows, C, ...] tensors;
    NaN if any block holds one."""
    out, ref = out.double().reshape(rows, out.shape[1], -1), ref.double().reshape(rows, ref.shape[1], -1)
    errs = []
    for c0 in range(0, out.shape[1], 64):
        o, r = out[:, c0:c0 + 64].flatten(1), ref[:, c0:c0 + 64].flatten(1)
        errs.append((o - r).norm(dim=1) / r.norm(dim=1).clamp_min(1e-30))
    return torch.cat(errs).max().item()           # torch's max propagates NaN


class Slice:
    """A C-channel slice of an [N, H, W, cs] buffer in storage type dt.  Small buffers are NaN outside
    (and, unless ``value`` is given, inside) the slice; a 4.5 GiB one comes from torch.empty and only the
    slice and MARGIN channels each side of it are written."""

    def __init__(self, N, H, W, C, cs, dt, value=None):
        from stfunet.nhwc import Feat
        self.big = N * H * W * cs * 2 > V.LIMIT
        self.off = off = 8 if cs >= C + 8 else 0
        self.lo, self.hi = (max(0, off - MARGIN), min(cs, off + C + MARGIN)) if self.big else (0, cs)
        self.buf = torch.empty(N * H * W * cs, dtype=dt, device=DEV)
        self.v = self.buf.view(N, H, W, cs)
        if self.big:
            self.v[..., self.lo:self.hi] = float("nan")
        else:
            self.buf.fill_(float("nan"))
        if value is not None:                        # [N, C, H, W]
            self.v[..., off:off + C] = value.permute(0, 2, 3, 1)
        self.before = self.v[..., self.lo:self.hi].clone()
        self.C = C
        self.feat = Feat(self.buf, N, H, W, C, cs, off)

    def dense(self):
        return self.v[..., self.off:self.off + self.C].permute(0, 3, 1, 2).contiguous()

    def untouched_outside(self):
        now, a, b = self.v[..., self.lo:self.hi].view(torch.int16), self.off - self.lo, self.off - self.lo + self.C
        was = self.before.view(torch.int16)
        return torch.equal(now[..., :a], was[..., :a]) and torch.equal(now[..., b:], was[..., b:])


def launch(name, *args, **kw):
    """nhwc.igemm(*args, **kw), once, after asserting that the router names ``name`` for the arguments as
    they are at the launch (statistics, workspace and epilogue pointers set).  Returns igemm's result and
    whether the launch ran split over K."""
    from stfunet import _lib, nhwc
    real, seen = nhwc._launch, []

    def checked(fn, a, info):
        got = _lib.load().stf_igemm_kernel_name(ctypes.byref(a)).decode()
        assert fn == "stf_igemm" and got == name, (got, name)
        seen.append(bool(a.ws))
        return real(fn, a, info)
    nhwc._launch = checked
    try:
        res = nhwc.igemm(*args, **kw)
    finally:
        nhwc._launch = real
    assert len(seen) == 1
    return res, seen[0]


def conv_reference(d, x, wm, bias, dev):
    """float64 result [N, Cout, Ho, Wo] of the gather the signature describes, from the GEMM rows
    wm [Nout][R][S][Cs] the kernel reads: conv2d, the ConvT 2x2 scatter as conv_transpose2d (row
    (dy * 2 + dx) * Cout + co), the transposed gather as the input gradient of conv2d."""
    x, wm = x.double().to(dev), wm.double().to(dev)
    b = bias.double().to(dev) if bias is not None else None
    Nout, Cs = d["Nout"], d["Cs"]
    if d["scatter"]:
        return F.conv_transpose2d(x, wm.view(2, 2, Nout // 4, Cs).permute(3, 2, 0, 1), b, stride=2)
    if d["transposed"]:
        z = torch.zeros(d["N"], Nout, d["Hd"], d["Wd"], dtype=torch.float64, device=dev, requires_grad=True)
        y = F.conv2d(z, wm.permute(3, 0, 1, 2), stride=d["stride"], padding=d["pad"])
        assert y.shape == x.shape
        g = torch.autograd.grad(y, z, x)[0]
        return g + b[None, :, None, None] if b is not None else g
    return F.conv2d(x, wm.permute(0, 3, 1, 2), b, stride=d["stride"], padding=d["pad"])


def run_conv(s, dt, name, ycs=None):
    """One launch of signature ``s`` (EPI 0) checked against float64; ``ycs``: channel stride of the fused
    BN-backward y (default dense).  Returns whether it ran split over K."""
    from stfunet import _lib, nhwc
    from stfunet.nhwc import BNState
    d = V.fields(s)
    assert not d["lstm"] and not d["dst_low"] and d["S"] == d["R"]
    N, Cs, Nout, R, groups = d["N"], d["Cs"], d["Nout"], d["R"], d["groups"]
    Cout = Nout // 4 if d["scatter"] else Nout
    Ho, Wo = (2 * d["Hd"], 2 * d["Wd"]) if d["scatter"] else (d["Hd"], d["Wd"])
    with _lib.storage(dt):
        torch.full((16 << 20,), float("nan"), device=DEV)     # NaN blocks back in the caching allocator
        x = torch.randn(N, Cs, d["Hs"], d["Ws"], device=DEV).to(dt)
        wm = (torch.randn(Nout, R, R, Cs, device=DEV) / (R * R * Cs) ** 0.5).to(dt)
        bias = torch.randn(Cout, device=DEV) if d["bias"] else None
        base = torch.randn(N, Cout, Ho, Wo, device=DEV).to(dt) if d["acc"] else None
        ref = f64(lambda dev: conv_reference(d, x, wm, bias, dev))
        if base is not None:
            ref = ref + base.double()
        src = Slice(N, d["Hs"], d["Ws"], Cs, d["scs"], dt, x)
        kw = dict(transposed=bool(d["transposed"]), bias=bias, want_stats=bool(d["stats"]),
                  scatter2x2=bool(d["scatter"]), groups=groups, accumulate=bool(d["acc"]))
        geo = (Nout, R, R, d["stride"], d["pad"])
        plain = None
        if d["bnr"]:
            # dz must be bit-equal to the same launch without the fused reduction
            plain = Slice(N, Ho, Wo, Cout, d["dcs"], dt, base)
            nhwc.igemm(src.feat, wm.view(-1), geo[0], plain.feat, *geo[1:], **kw)
            y = Slice(N, Ho, Wo, Cout, ycs or Cout, dt, (torch.randn(N, Cout, Ho, Wo, device=DEV) * 2 + 0.5).to(dt))
            st = BNState(Cout, DEV, N * Ho * Wo, groups)
            st.mean.copy_(torch.randn(groups, Cout, device=DEV) * 0.3 + 0.5)
            st.invstd.copy_(torch.rand(groups, Cout, device=DEV) + 0.5)
            st.scale.copy_(torch.randn(groups, Cout, device=DEV))
            st.shift.copy_(torch.randn(groups, Cout, device=DEV) * 0.5)
            kw["bnr"] = (y.feat, st, True)
        dst = Slice(N, Ho, Wo, Cout, d["dcs"], dt, base)
        (stats, tiles), split = launch(name, src.feat, wm.view(-1), geo[0], dst.feat, *geo[1:], **kw)
        torch.cuda.synchronize()
        out = dst.dense()
        assert torch.isfinite(out).all(), "unwritten or non-finite outputs"
        err = worst_rel(out, ref, N)
        print(f"{name} {_id(dt)}: output {err:.3e}")
        assert err <= BOUND_16[dt]
        assert dst.untouched_outside(), "channels outside the destination slice changed"
        og = out.double().view(groups, N // groups, Cout, Ho, Wo)
        if d["stats"]:
            got = stats.view(groups, tiles, 2, Nout).double().sum(1)
            assert torch.isfinite(got).all()
            e1 = worst_rel(got[:, 0], og.sum((1, 3, 4)), groups)
            e2 = worst_rel(got[:, 1], (og * og).sum((1, 3, 4)), groups)
            print(f"  statistics {e1:.3e} {e2:.3e}")
            assert e1 <= BOUND_STATS[dt] and e2 <= BOUND_STATS[dt]
        if d["bnr"]:
            assert torch.equal(out.view(torch.int16), plain.dense().view(torch.int16))
            got = stats.view(groups, tiles, 2, Nout).double().sum(1)
            assert torch.isfinite(got).all()
            yy = y.dense().double().view(groups, N // groups, Cout, Ho, Wo)
            b5 = lambda t: t.double()[:, None, :, None, None]      # noqa: E731
            g = og * ((yy * b5(st.scale) + b5(st.shift)) > 0)
            xh = (yy - b5(st.mean)) * b5(st.invstd)
            e1 = worst_rel(got[:, 0], g.sum((1, 3, 4)), groups)
            e2 = worst_rel(got[:, 1], (g * xh).sum((1, 3, 4)), groups)
            print(f"  BN-backward partials {e1:.3e} {e2:.3e}")
            assert e1 <= BOUND_BNR and e2 <= BOUND_BNR
            assert y.untouched_outside()
    return split


# ------------------------------------------------------------------ LSTM epilogues
def lstm_cell64(x, wm, bias, c_prev, dh, dc_next, c_t=None):
    """float64 cell of oracle/stf.py's lstm_last_hidden on GEMM rows 4c + q (gate q of i, f, g, o of
    hidden channel c) and its backward (csrc/common.h's lstm_cell_bwd written out); ``c_t``: the stored
    cell the backward reads (default: the one computed here)."""
    M = x.shape[0]
    pre = (x @ wm.t() + bias).view(M, -1, 4)
    gi, gf, go = torch.sigmoid(pre[..., 0]), torch.sigmoid(pre[..., 1]), torch.sigmoid(pre[..., 3])
    gg = torch.tanh(pre[..., 2])
    c = gf * c_prev + gi * gg
    h = go * torch.tanh(c)
    tc = torch.tanh(c if c_t is None else c_t)
    dct = dh * go * (1 - tc * tc) + dc_next
    dg = torch.stack([dct * gg * gi * (1 - gi), dct * c_prev * gf * (1 - gf), dct * gi * (1 - gg * gg),
                      dh * tc * go * (1 - go)], -1)
    return {"gates": torch.stack([gi, gf, gg, go], -1).flatten(1), "c_out": c, "h_out": h,
            "dgates": dg.flatten(1), "dc_prev": dct * gf}


def lstm_operands(M, C, gen=None, device="cpu"):
    r = lambda *sh: torch.randn(*sh, generator=gen, device=device, dtype=torch.float32)      # noqa: E731
    return dict(x=r(M, 2 * C), wm=r(4 * C, 2 * C) / (2 * C) ** 0.5, bias=r(4 * C), c_prev=r(M, C), dh=r(M, C),
                dc_next=r(M, C))


def lstm_emulation_error(dt, M=3 * 9 * 11, C=32):
    """Relative L2 error, per output, of a float64 cell fed the operands rounded as the kernel stores them
    (x, weights, dh in ``dt``; bias, c_prev, dc_next fp32) with its outputs rounded to their storage
    (h, dgates ``dt``; gates, c, dc_prev fp32), against the float64 cell of the unrounded operands."""
    ops = lstm_operands(M, C, torch.Generator().manual_seed(0))
    exact = lstm_cell64(**{k: v.double() for k, v in ops.items()})
    rounded = {k: (v.to(dt) if k in ("x", "wm", "dh") else v).double() for k, v in ops.items()}
    emu = lstm_cell64(**rounded)
    emu = {k: (v.to(dt) if k in ("h_out", "dgates") else v.float()).double() for k, v in emu.items()}
    return {k: ((emu[k] - exact[k]).norm() / exact[k].norm()).item() for k in exact}


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_lstm_bounds_are_twice_the_emulation_error(dt):
    """The LSTM epilogues' bound (no kernel-level bound existed).  Measured with lstm_emulation_error():
    a float64 cell fed the 16-bit-rounded operands, its outputs rounded to their storage, against the
    float64 cell of the unrounded operands (297 pixels, 32 hidden channels, seed 0), relative L2:

        bf16  gates 1.33e-3  c_out 1.41e-3  h_out 2.38e-3  dgates 2.72e-3  dc_prev 1.07e-3
        fp16  gates 1.63e-4  c_out 1.71e-4  h_out 2.98e-4  dgates 3.30e-4  dc_prev 1.35e-4

    BOUND_LSTM is twice that, for the accumulation order (recomputed and compared here), applied per
    image and 64-column slice against the float64 cell of the *same* 16-bit operands (the kernels
    measure 6e-8 .. 8e-8 on the fp32 outputs and the storage rounding on the 16-bit ones: bf16 1.7e-3,
    fp16 2.1e-4).  The backward epilogue (EPI 2) writes dgates and dc_prev only; the cell it recomputes is
    checked through them."""
    meas = lstm_emulation_error(dt)
    for k, v in meas.items():
        assert 1.9 * v <= BOUND_LSTM[dt][k] <= 2.1 * v, (k, v)


def run_lstm(s, dt, name):
    from stfunet import _lib, nhwc
    from stfunet._lib import LstmEpi
    from stfunet.nhwc import _p
    d = V.fields(s)
    N, hw, C, backward = d["N"], d["Hs"] * d["Ws"], d["Nout"] // 4, d["lstm"] == 2
    M = N * hw
    assert d["Cs"] == 2 * C and d["R"] == 1 and d["dcs"] == d["scs"]
    with _lib.storage(dt):
        torch.full((16 << 20,), float("nan"), device=DEV)
        ops = lstm_operands(M, C, device=DEV)
        x, wm, dh = ops["x"].to(dt), ops["wm"].to(dt), ops["dh"].to(dt)
        as_img = lambda t: t.view(N, d["Hs"], d["Ws"], -1).permute(0, 3, 1, 2)      # noqa: E731
        src = Slice(N, d["Hs"], d["Ws"], 2 * C, d["scs"], dt, as_img(x))
        ref = lstm_cell64(x.double(), wm.double(), ops["bias"].double(), ops["c_prev"].double(), dh.double(),
                          ops["dc_next"].double())
        nan32 = lambda *sh: torch.full(sh, float("nan"), device=DEV)      # noqa: E731
        if not backward:
            out = {"gates": nan32(M, 4 * C), "c_out": nan32(M, C)}
            hs = Slice(N, d["Hs"], d["Ws"], C, C + 16, dt)
            epi = LstmEpi(_p(ops["c_prev"]), _p(out["c_out"]), hs.feat.ptr(), hs.feat.cs, _p(out["gates"]))
        else:
            # the backward reads the stored fp32 cell c_t and recomputes the gates from the same GEMM
            c_t = ref["c_out"].float()
            ref = lstm_cell64(x.double(), wm.double(), ops["bias"].double(), ops["c_prev"].double(), dh.double(),
                              ops["dc_next"].double(), c_t.double())
            out = {"dc_prev": nan32(M, C), "dgates": torch.full((M, 4 * C), float("nan"), device=DEV, dtype=dt)}
            dhs = Slice(N, d["Hs"], d["Ws"], C, C + 16, dt, as_img(dh))
            epi = LstmEpi(_p(ops["c_prev"]), _p(c_t), None, 0, None, 1, dhs.feat.ptr(), dhs.feat.cs,
                          _p(ops["dc_next"]), _p(out["dc_prev"]), _p(out["dgates"]))
        launch(name, src.feat, wm.view(-1), 4 * C, src.feat, 1, 1, 1, 0, bias=ops["bias"], lstm=epi)
        torch.cuda.synchronize()
        if not backward:
            out["h_out"] = hs.dense()
            assert hs.untouched_outside()
        assert src.untouched_outside()
        assert torch.equal(src.dense().view(torch.int16), as_img(x).contiguous().view(torch.int16))
        for k, v in out.items():
            v = v if v.dim() == 4 else as_img(v)
            assert torch.isfinite(v).all(), k
            err = worst_rel(v, as_img(ref[k]), N)
            print(f"{name} {_id(dt)}: {k} {err:.3e}")
            assert err <= BOUND_LSTM[dt][k], k


def run(s, dt, name):
    return run_lstm(s, dt, name) if V.fields(s)["lstm"] else run_conv(s, dt, name)


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("name,s", V.cases(),
                         ids=[f"{n.replace(' ', '')}-{'x'.join(map(str, s[:4]))}" for n, s in V.cases()])
def test_variant_parity(name, s, dt):
    """Every reachable variant below 4 GiB: outputs, statistics, fused BN-backward partials, the LSTM
    epilogues (bounds: test_lstm_bounds_are_twice_the_emulation_error), nothing unwritten, nothing outside
    the slice."""
    run(s, dt, name)


# ------------------------------------------------------------------ 4 GiB and more
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("name", list(V.SRC_4GIB))
def test_source_of_4gib(name, dt):
    """The register-staged kernels without SMALLC, the 64-bit-addressing fallback: a 32-channel slice of
    a 4.5 GiB source whose last image lies wholly past byte offset 2^32."""
    for s in V.SRC_4GIB[name]:
        assert V.src_bytes(s) >= 1 << 32
        run(s, dt, name)


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("label,s,name", V.DST_4GIB, ids=[c[0].replace(" ", "_") for c in V.DST_4GIB])
def test_destination_of_4gib(label, s, name, dt):
    """A 64- or 128-channel slice of a 4.5 GiB destination, the source small: one launch per kernel family
    a dense destination of the same shape selects.  The tile kernels store through a 32-bit buffer
    descriptor over the whole destination, so these launches must run (and be right on) the linear
    kernels, which address the destination with 64 bits."""
    assert V.dst_bytes(s) >= 1 << 32
    split = run_conv(s, dt, name)
    assert split == (label == "split-K")


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_bn_backward_y_of_4gib(dt):
    """A BN-backward-fused dgrad whose y is a slice of a 4.5 GiB buffer (dz dense)."""
    s, ycs, name = V.BNR_Y_4GIB
    run_conv(s, dt, name, ycs=ycs)
