"""Every kernel stf_wgrad can select, its split-K plan and stf_wgrad_reduce, against float64 -- exactly.

The cases are tests/_wgrad_variants.py's table (tests/test_wgrad_variants_cpu.py checks that it names every
kernel the router returns and that every case has the edge it is there for) in both storage types, through
the C ABI, so the test owns the workspace.

Operands are integers in [-3, 3], exact in bf16 and fp16: every product is an integer of magnitude <= 9 and
every partial sum, in any order, an integer below 2^24 (N * Hd * Wd * 9 < 2^24, asserted on the CPU), so
fp32 accumulation, the slabs and the reduce's double fold are all exact and the result must EQUAL the
float64 weight gradient of conv2d (conv_transpose2d with the operand roles swapped for the ConvT-shaped
launches).  A dropped, duplicated or shifted pixel, a tap read across a row end, a misplaced tile or a
transposition in the reduce changes an integer.  x and dy are channel slices of NaN-filled buffers with one
NaN image before and after the tensor the kernel is given, the workspace is ws_bytes of NaN between
sentinels (a slab's worth, at least 4096 floats, each side) and so is the output: a read outside the operands
poisons a sum, an unwritten slab float stays NaN, a write outside the slabs or the output changes a sentinel.

The same cases run once more with Gaussian operands rounded to the storage type, against the any-order
fp32 summation bound |out - ref| <= M * 2^-23 * A per element (M = N * Hd * Wd pixels, A the same gradient
of the operands' absolute values; one ulp of slack per addition, so a truncating adder passes, accumulation
or slab folding below fp32 does not).  Each prints its largest err / bound.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _wgrad_variants as W

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
GUARD = 4096                        # sentinel floats each side of the workspace and of the output, at least
SENTINEL = 0x7FC0BEEF               # their bits (a NaN nothing computes)
MARGIN = 8                          # NaN channels each side of a slice of a 4.5 GiB buffer
NAN = float("nan")
_REFS = {}                          # (signature, operand kind[, storage type]) -> (x, dy, reference, bound)
WORST = {}                          # (kernel, storage type) -> largest err / bound of the Gaussian runs so far


def _id(v):
    return "bf16" if v is torch.bfloat16 else "fp16" if v is torch.float16 else None


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


def f64(fn):
    """fn(device) in float64 on the GPU where torch has the ops there, else on the CPU; result on the GPU."""
    try:
        return fn(DEV).to(DEV)
    except RuntimeError:
        return fn("cpu").to(DEV)


def weight_gradient(d, x, dy, dev):
    """float64 dW [Nout, Cs, R, R] of x [N, Cs, Hs, Ws] and dy [N, Nout, Hd, Wd]: autograd of conv2d, or,
    for the launches shaped like ConvTranspose2d(2, 2)'s (dy the small grid, x the 2x larger tensor), of
    conv_transpose2d with the operand roles swapped."""
    x, dy = x.double().to(dev), dy.double().to(dev)
    R, st = d["R"], d["stride"]
    if R == 2 and st == 2 and d["pad"] == 0 and (d["Hs"], d["Ws"]) == (2 * d["Hd"], 2 * d["Wd"]):
        w = torch.zeros(d["Nout"], d["Cs"], 2, 2, dtype=torch.float64, device=dev, requires_grad=True)
        y = F.conv_transpose2d(dy, w, stride=2)
        assert y.shape == x.shape
        return torch.autograd.grad(y, w, x)[0]
    w = torch.zeros(d["Nout"], d["Cs"], R, R, dtype=torch.float64, device=dev, requires_grad=True)
    y = F.conv2d(x, w, stride=st, padding=d["pad"])
    assert y.shape == dy.shape
    return torch.autograd.grad(y, w, dy)[0]


def operands(s, kind, dt):
    """(x [N, Cs, Hs, Ws], dy [N, Nout, Hd, Wd], float64 reference [Nout, Cs, R, R], bound or None), computed
    once per signature: integers in [-3, 3] (the same for both storage types) or Gaussians rounded to ``dt``."""
    key = (s, kind) if kind == "int" else (s, kind, dt)
    if key not in _REFS:
        d = W.fields(s)
        gen = torch.Generator().manual_seed(hash(s) & 0xFFFFFF)
        xs, ds = (d["N"], d["Cs"], d["Hs"], d["Ws"]), (d["N"], d["Nout"], d["Hd"], d["Wd"])
        if kind == "int":
            x, dy = (torch.randint(-3, 4, sh, generator=gen, dtype=torch.int8).to(DEV) for sh in (xs, ds))
            bound = None
        else:
            x, dy = (torch.randn(sh, generator=gen).to(dt).to(DEV) for sh in (xs, ds))
            M = d["N"] * d["Hd"] * d["Wd"]
            bound = f64(lambda dev: weight_gradient(d, x.abs(), dy.abs(), dev)) * (M * 2.0 ** -23)
        _REFS[key] = (x, dy, f64(lambda dev: weight_gradient(d, x, dy, dev)), bound)
    return _REFS[key]


class Operand:
    """C channels at channel ``off`` of [N, H, W] pixels with ``cs``-wide rows, in storage type dt, holding
    ``value`` [N, C, H, W].  The buffer is NaN everywhere else and has one NaN image before and after the
    N the kernel is given; a 4.5 GiB one comes from torch.empty, without the two images, and only the slice
    and MARGIN channels each side of it are written."""

    def __init__(self, N, H, W_, C, cs, off, dt, value):
        img = H * W_ * cs
        big = N * img * 2 > W.LIMIT
        first = 0 if big else img
        self.buf = torch.empty((N + (0 if big else 2)) * img, dtype=dt, device=DEV)
        v = self.buf[first:first + N * img].view(N, H, W_, cs)
        if big:
            v[..., max(0, off - MARGIN):min(cs, off + C + MARGIN)] = NAN
        else:
            self.buf.fill_(NAN)
        stored = value.permute(0, 2, 3, 1).to(dt)
        assert torch.equal(stored.double(), value.permute(0, 2, 3, 1).double()), "operand not exact in the storage type"
        v[..., off:off + C] = stored
        self.ptr = self.buf.data_ptr() + 2 * (first + off)
        self.rows = self.buf[first:]                  # for nhwc.Feat: the N images and what follows


def guarded(n, guard):
    """n NaN floats between ``guard`` sentinel floats each side."""
    buf = torch.full((guard + n + guard,), NAN, device=DEV)
    bits = buf.view(torch.int32)
    bits[:guard] = SENTINEL
    bits[guard + n:] = SENTINEL
    return buf


def sentinels_intact(buf, n, guard):
    bits = buf.view(torch.int32)
    return bool((bits[:guard] == SENTINEL).all()) and bool((bits[guard + n:] == SENTINEL).all())


def wgrad_args(d, xo, dyo, grid_blocks):
    from stfunet import _lib
    g = _lib.ConvGeom(d["N"], d["Hs"], d["Ws"], d["Cs"], d["xcs"], d["Hd"], d["Wd"], d["R"], d["R"], d["stride"],
                      d["pad"], 0)
    return _lib.WgradArgs(g, dyo.ptr, d["dycs"], d["Nout"], xo.ptr, None, 0, grid_blocks)


def launch(lib, a, d, splits, nbytes):
    """stf_wgrad into a fresh guarded workspace, then stf_wgrad_reduce into a fresh guarded output.  Returns
    the slabs [splits, Nout, R, S, Cs] and the output [Nout, Cs, R, S] after checking that both calls return
    0, every slab float is finite and no sentinel changed."""
    from stfunet import _lib
    Nout, R, Cs = d["Nout"], d["R"], d["Cs"]
    total = Nout * R * R * Cs
    assert nbytes % 16 == 0
    wguard = max(GUARD, total)                        # a slab too many lands in the sentinels
    ws, out = guarded(nbytes // 4, wguard), guarded(total, GUARD)
    a.ws, a.splits = ws.data_ptr() + 4 * wguard, splits
    assert lib.stf_wgrad(ctypes.byref(a), _lib.stream()) == 0
    torch.cuda.synchronize()
    assert sentinels_intact(ws, nbytes // 4, wguard), "written outside the workspace stf_wgrad_plan asked for"
    assert nbytes == splits * total * 4
    slabs = ws[wguard:wguard + splits * total].view(splits, Nout, R, R, Cs)
    assert torch.isfinite(slabs).all(), "slab floats unwritten or not finite"
    assert lib.stf_wgrad_reduce(a.ws, splits, Nout, R, R, Cs, out.data_ptr() + 4 * GUARD, _lib.stream()) == 0
    torch.cuda.synchronize()
    assert sentinels_intact(out, total, GUARD), "written outside the output"
    assert sentinels_intact(ws, nbytes // 4, wguard), "the reduce wrote to the workspace's sentinels"
    return slabs, out[GUARD:GUARD + total].view(Nout, Cs, R, R)


def run(s, dt, name, kind):
    from stfunet import _lib
    d = W.fields(s)
    with _lib.storage(dt):
        lib = _lib.load()
        torch.full((16 << 20,), NAN, device=DEV)      # NaN blocks back in the caching allocator
        x, dy, ref, bound = operands(s, kind, dt)
        xo = Operand(d["N"], d["Hs"], d["Ws"], d["Cs"], d["xcs"], d["xoff"], dt, x)
        dyo = Operand(d["N"], d["Hd"], d["Wd"], d["Nout"], d["dycs"], d["dyoff"], dt, dy)
        a = wgrad_args(d, xo, dyo, d["grid_blocks"])
        assert lib.stf_wgrad_kernel_name(ctypes.byref(a)).decode() == name
        sp, nb = ctypes.c_int(0), ctypes.c_size_t(0)
        assert lib.stf_wgrad_plan(ctypes.byref(a), ctypes.byref(sp), ctypes.byref(nb)) == 0
        slabs, out = launch(lib, a, d, sp.value, nb.value)
        folded = slabs.double().sum(0).permute(0, 3, 1, 2)        # [Nout][R][S][Cs] -> [Nout][Cs][R][S]
        if kind == "int":
            assert torch.equal(folded, ref), f"slabs: {(folded != ref).sum().item()} of {ref.numel()} differ"
            assert torch.equal(out.double(), ref), f"output: {(out.double() != ref).sum().item()} of {ref.numel()} differ"
        else:
            worst = 0.0
            for got in (folded, out.double()):
                err = (got - ref).abs()
                worst = max(worst, (err / bound.clamp_min(1e-300)).max().item())
                assert (err <= bound).all(), f"err / bound up to {worst:.3e}"
            key = (name, _id(dt))
            WORST[key] = max(WORST.get(key, 0.0), worst)
            print(f"{name} {_id(dt)} {W.case_id(name, s)}: err / bound {worst:.3e} (kernel's largest so far "
                  f"{WORST[key]:.3e})")
        slabs2, out2 = launch(lib, a, d, sp.value, nb.value)
        assert torch.equal(slabs2.view(torch.int32), slabs.view(torch.int32))
        assert torch.equal(out2.view(torch.int32), out.view(torch.int32)), "not repeatable bit for bit"
    return out


CASES = [(n, s) for n, s, _ in W.cases()]
IDS = [W.case_id(n, s) for n, s in CASES]


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("name,s", CASES, ids=IDS)
def test_integer_operands_give_the_float64_gradient_exactly(name, s, dt):
    run(s, dt, name, "int")


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("name,s", CASES, ids=IDS)
def test_gaussian_operands_within_the_fp32_summation_bound(name, s, dt):
    """Measured err / bound, largest per kernel over its cases (MI355X): see DESIGN.md's test section."""
    run(s, dt, name, "gauss")


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("taps", [1, 4, 9, 49])
def test_reduce_alone(taps, dt):
    """stf_wgrad_reduce over synthetic integer slabs [splits][Nout][R][S][Cs]: the per-tap kernel's rounds of
    four and its remainder loop (splits up to 8, for 1, 4 and 9 taps) and the generic kernel (more splits, or
    49 taps) equal the float64 sum, transposed to [Nout][Cs][R][S]."""
    from stfunet import _lib
    R = {1: 1, 4: 2, 9: 3, 49: 7}[taps]
    Nout, Cs = 24, 40
    total = Nout * taps * Cs
    gen = torch.Generator().manual_seed(taps)
    with _lib.storage(dt):
        lib = _lib.load()
        for splits in (1, 2, 3, 4, 5, 7, 8, 9, 13):
            vals = torch.randint(-1000, 1001, (splits, Nout, R, R, Cs), generator=gen).to(DEV)
            ws, out = guarded(splits * total, GUARD), guarded(total, GUARD)      # a slab too many reads NaN
            ws[GUARD:GUARD + splits * total] = vals.float().view(-1)
            rc = lib.stf_wgrad_reduce(ws.data_ptr() + 4 * GUARD, splits, Nout, R, R, Cs, out.data_ptr() + 4 * GUARD,
                                      _lib.stream())
            torch.cuda.synchronize()
            assert rc == 0
            got = out[GUARD:GUARD + total].view(Nout, Cs, R, R).double()
            assert torch.equal(got, vals.double().sum(0).permute(0, 3, 1, 2)), splits
            assert sentinels_intact(out, total, GUARD), splits
            assert torch.equal(ws[GUARD:GUARD + splits * total].view(splits, Nout, R, R, Cs), vals.float()), splits


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("name", list(W.WIDE_4GIB), ids=[W.case_id(n, s) for n, s in W.WIDE_4GIB.items()])
def test_operand_of_4gib(name, dt):
    """x (dy for the 8-channel kernel) a 64- or 128-channel slice of a 4.5 GiB buffer whose last image lies
    wholly past byte offset 2^32, the other operand small: integer operands, equality."""
    run(W.WIDE_4GIB[name], dt, name, "int")


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("name", [W.C8, W.F16, W.T16_2])
def test_side_stream_wgrad_equals_the_direct_call(name, dt):
    """nhwc.wgrad the way the training step calls it -- WGRAD_STREAM set: grid_blocks = the CU count, the
    event hand-off to the side stream and back, a workspace from the pool -- bit for bit the direct call
    with that grid_blocks, and exactly the float64 gradient (one case per fused family)."""
    from stfunet import _lib, nhwc
    from stfunet.nhwc import Feat
    (s,) = [s for s, p in W.TABLE[name] if "cus" in p]
    d = W.fields(s)
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    s = s[:-1] + (cus,)
    direct = run(s, dt, name, "int")
    with _lib.storage(dt):
        torch.full((16 << 20,), NAN, device=DEV)
        x, dy, ref, _ = operands(s, "int", dt)
        xo = Operand(d["N"], d["Hs"], d["Ws"], d["Cs"], d["xcs"], d["xoff"], dt, x)
        dyo = Operand(d["N"], d["Hd"], d["Wd"], d["Nout"], d["dycs"], d["dyoff"], dt, dy)
        fx = Feat(xo.rows, d["N"], d["Hs"], d["Ws"], d["Cs"], d["xcs"], d["xoff"])
        fdy = Feat(dyo.rows, d["N"], d["Hd"], d["Wd"], d["Nout"], d["dycs"], d["dyoff"])
        out = torch.full((ref.numel(),), NAN, device=DEV)
        main, side = torch.cuda.current_stream(), nhwc.side_stream(DEV, "wgrad")
        real, seen = nhwc._launch, []

        def recorded(fn, a, info):
            seen.append((fn, a.grid_blocks, _lib.stream()))
            return real(fn, a, info)
        nhwc._launch, nhwc.WGRAD_STREAM, nhwc.WGRAD_MAIN = recorded, side, main
        try:
            nhwc.wgrad(fdy, fx, d["R"], d["R"], d["stride"], d["pad"], out)
        finally:
            nhwc._launch, nhwc.WGRAD_STREAM, nhwc.WGRAD_MAIN = real, None, None
        assert seen == [("stf_wgrad", cus, side.cuda_stream)] and _lib.stream() == main.cuda_stream
        main.wait_stream(side)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), direct.reshape(-1).view(torch.int32))
        assert torch.equal(out.view_as(ref).double(), ref)

