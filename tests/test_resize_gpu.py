"""The logits resize kernels (stf_resize_bilinear_fwd / _bwd, csrc/resize.hip) through
``stfunet.upsample_logits``, against torch on the CPU.

Tolerances (rtol = 0 throughout), with u = 2^-24:
  * forward vs fp32 ``F.interpolate``: the indices and weights follow the same formula, only the
    evaluation order of the two lerps may differ; each side makes at most ~6 roundings on
    magnitudes <= max|x|: atol = 16 u max|x|.  The identity case is bit-exact; the exact-2x case
    (weights exactly 0.25 / 0.75) is also held against fp64 at the same atol.
  * backward vs torch CPU autograd: per source pixel the weights sum to at most
    (H/h)(W/w) <= 4.5 over at most 16 terms, two fp32 summation orders differ by at most about
    2 * 15 * u * 4.5 * max|dy|: atol = 160 u max|dy|.  The single-source-pixel case sums every
    output of its plane: fp64 ``dy.sum()`` per plane, atol = 12 u sum|dy|.
  * transpose identity in fp64 on the host: |<fwd(x), dy> - <x, bwd(dy)>| <= 1e-6 |fwd(x)|.|dy|,
    which catches a range bound that drops or doubles a contribution.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
CASES = [((16, 16), (32, 32)),      # exact 2x
         ((34, 36), (66, 70)),      # what the model produces for a 66x70 frame: ratio not 2
         ((13, 9), (27, 20)),       # odd and unequal ratios
         ((5, 7), (5, 7)),          # identity
         ((1, 1), (4, 3))]          # a single source pixel
IDS = ["2x", "model66x70", "odd", "identity", "single"]
_CACHE = {}


def case(lo, hi):
    """x, dy, the CPU references (made once per case, never modified) and the device results."""
    key = (lo, hi)
    if key not in _CACHE:
        from stfunet import upsample_logits
        g = torch.Generator().manual_seed(100 * lo[0] + hi[1])
        x = torch.randn(2, 3, *lo, generator=g) * 8
        dy = torch.randn(2, 3, *hi, generator=g)
        xr = x.clone().requires_grad_(True)
        ref = F.interpolate(xr, size=hi, mode="bilinear", align_corners=False)
        ref.backward(dy)
        xd = x.to(DEV).requires_grad_(True)
        y = upsample_logits(xd, hi)
        y.backward(dy.to(DEV))
        torch.cuda.synchronize()
        _CACHE[key] = dict(x=x, dy=dy, ref=ref.detach(), ref_dx=xr.grad, y=y.detach().cpu(), dx=xd.grad.cpu())
    return _CACHE[key]


@pytest.mark.parametrize("lo,hi", CASES, ids=IDS)
def test_forward_against_torch_cpu(lo, hi):
    c = case(lo, hi)
    assert c["y"].shape == (2, 3, *hi) and c["y"].dtype == torch.float32
    atol = 16 * U * c["x"].abs().max().item()
    err = (c["y"] - c["ref"]).abs().max().item()
    print(f"{lo}->{hi}: forward max err {err:.3e} (atol {atol:.3e})")
    assert err <= atol
    if lo == hi:
        assert torch.equal(c["y"], c["x"])
    if (2 * lo[0], 2 * lo[1]) == hi:
        ref64 = F.interpolate(c["x"].double(), size=hi, mode="bilinear", align_corners=False)
        err64 = (c["y"].double() - ref64).abs().max().item()
        print(f"{lo}->{hi}: forward max err vs fp64 {err64:.3e}")
        assert err64 <= atol


@pytest.mark.parametrize("lo,hi", CASES, ids=IDS)
def test_backward_against_torch_cpu(lo, hi):
    c = case(lo, hi)
    assert c["dx"].shape == c["x"].shape
    if lo == (1, 1):
        ref = c["dy"].double().sum((2, 3), keepdim=True)
        atol = 12 * U * c["dy"].double().abs().sum((2, 3)).max().item()
        err = (c["dx"].double() - ref).abs().max().item()
    else:
        atol = 160 * U * c["dy"].abs().max().item()
        err = (c["dx"] - c["ref_dx"]).abs().max().item()
    print(f"{lo}->{hi}: backward max err {err:.3e} (atol {atol:.3e})")
    assert err <= atol
    if lo == hi:
        assert torch.equal(c["dx"], c["dy"])


@pytest.mark.parametrize("lo,hi", CASES, ids=IDS)
def test_backward_is_the_forwards_transpose(lo, hi):
    c = case(lo, hi)
    y, dy, x, dx = (c[k].double() for k in ("y", "dy", "x", "dx"))
    lhs, rhs = (y * dy).sum().item(), (x * dx).sum().item()
    bound = 1e-6 * (y.abs() * dy.abs()).sum().item()
    print(f"{lo}->{hi}: <fwd x, dy> {lhs:.9e}  <x, bwd dy> {rhs:.9e}  bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound


def _direct(name, src, planes, a, b, dst, c, d, lib=None):
    from stfunet import _lib
    lib = lib or _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    return getattr(lib, name)(p(src), planes, a, b, p(dst), c, d, ctypes.c_void_p(_lib.stream()))


@pytest.mark.parametrize("lo,hi", CASES, ids=IDS)
def test_backward_deterministic_and_overwrites(lo, hi):
    c = case(lo, hi)
    dy = c["dy"].to(DEV)
    outs = []
    for fill in (float("nan"), 7.0):
        dx = torch.full((2, 3, *lo), fill, device=DEV)
        assert _direct("stf_resize_bilinear_bwd", dy, 6, hi[0], hi[1], dx, lo[0], lo[1]) == 0
        torch.cuda.synchronize()
        outs.append(dx.cpu())
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], c["dx"])


@pytest.mark.parametrize("lo,hi", CASES, ids=IDS)
def test_both_libraries_bit_identical(lo, hi):
    from stfunet import _lib, upsample_logits
    c = case(lo, hi)
    with _lib.storage(torch.float16):
        xd = c["x"].to(DEV).requires_grad_(True)
        y = upsample_logits(xd, hi)
        y.backward(c["dy"].to(DEV))
    assert torch.equal(y.detach().cpu(), c["y"]) and torch.equal(xd.grad.cpu(), c["dx"])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16lib", "fp16lib"])
def test_error_codes_without_a_launch(dtype):
    from stfunet import _lib
    lib = _lib.load(dtype)
    EINVAL = 100001
    x = torch.full((6, 4, 5), 3.0, device=DEV)
    y = torch.full((6, 8, 10), -5.0, device=DEV)
    for name, src, dst, (a, b), (c, d) in (("stf_resize_bilinear_fwd", x, y, (4, 5), (8, 10)),
                                           ("stf_resize_bilinear_bwd", y, x, (8, 10), (4, 5))):
        lo_first = name.endswith("fwd")
        sentinel = dst.clone()
        assert _direct(name, None, 6, a, b, dst, c, d, lib) == EINVAL             # NULL pointers
        assert _direct(name, src, 6, a, b, None, c, d, lib) == EINVAL
        assert _direct(name, src, 0, a, b, dst, c, d, lib) == EINVAL              # zero sizes
        assert _direct(name, src, 6, 0, b, dst, c, d, lib) == EINVAL
        assert _direct(name, src, 6, a, b, dst, c, 0, lib) == EINVAL
        # H < h / W < w: (4, 5) -> (3, 10) and (4, 5) -> (8, 4)
        small = ((a, b), (3, d)) if lo_first else ((3, b), (c, d))
        assert _direct(name, src, 6, *small[0], dst, *small[1], lib) == EINVAL
        small = ((a, b), (c, 4)) if lo_first else ((a, 4), (c, d))
        assert _direct(name, src, 6, *small[0], dst, *small[1], lib) == EINVAL
        # planes * H * W = 2^31 (32-bit index math); nothing runs, so the small buffers are never touched
        big = ((a, b), (1 << 15, 1 << 14)) if lo_first else ((1 << 15, 1 << 14), (c, d))
        assert _direct(name, src, 4, *big[0], dst, *big[1], lib) == EINVAL
        torch.cuda.synchronize()
        assert torch.equal(dst, sentinel), name
    with pytest.raises(ValueError, match="smaller"):
        from stfunet import upsample_logits
        upsample_logits(x.view(2, 3, 4, 5), (3, 9))
