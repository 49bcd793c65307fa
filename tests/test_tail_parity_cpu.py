"""The references and operand builders of tests/_tail_ref.py, checked without a GPU: against float64 torch autograd,
F.interpolate and F.max_pool2d; that every exact builder stays below 2^24 granules in every sum (so the GPU test
may ask for equality); that the Gaussian seeds leave at most 1e-4 of the ReLU decisions open; and that every case
of the tables has the edge it is listed for."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _bn_ref
import _tail_ref as T

f64 = torch.float64
DTS = [torch.bfloat16, torch.float16]
LIMIT = 2.0 ** 24


# ------------------------------------------------------------------ head
@pytest.mark.parametrize("identity", [False, True])
@pytest.mark.parametrize("K", T.HEAD_K)
@pytest.mark.parametrize("C", [8, 64])
def test_head_ref_is_autograd(C, K, identity):
    shape = N, H, W = (3, 9, 7)
    o = T.HeadOps(shape, C, K, "gauss", torch.bfloat16, identity)
    r = T.head_ref(o)
    z = T.nchw(o.y * o.scale + o.shift, N, H, W).requires_grad_(True)
    w, b = o.w.clone().requires_grad_(True), o.bias.clone().requires_grad_(True)
    logits = F.conv2d(F.relu(z), w.view(K, C, 1, 1), b)
    logits.backward(o.dl)
    g = T.nhwc(z.grad)
    close = lambda a, c: torch.allclose(a, c, rtol=1e-12, atol=1e-12)  # noqa: E731
    assert close(r["logits"], logits.detach()) and close(r["g"], g) and close(r["dW"], w.grad) and close(r["db"], b.grad)
    assert close(r["sums"][0], g.sum(0)) and close(r["sums"][1], (g * (o.y - o.mean) * o.invstd).sum(0))
    for k in ("logits", "g", "dW", "db", "sums"):
        assert r["b_" + k].shape == r[k].shape and bool((r["b_" + k] >= 0).all())


def _exact_ok(o):
    gr = T.head_granules(o)
    assert max(gr.values()) < LIMIT, gr
    assert gr["g"] <= 48                                  # |g| <= 4 classes x 3 x 4: exact in bf16 and fp16
    for v in (o.y, o.w, o.dl, o.bias, o.mean):
        assert torch.equal(v, v.round())
    for v in (o.scale, o.invstd, o.shift):               # multiples of 0.5: the granule
        assert torch.equal(v * 2, (v * 2).round())
    assert float(o.y.abs().max()) <= 8 and float(o.shift.abs().max()) <= 4
    return gr


@pytest.mark.parametrize("identity", [False, True])
@pytest.mark.parametrize("C", T.HEAD_C)
@pytest.mark.parametrize("shape", T.HEAD_GRID + [T.HEAD_PIXEL[0]], ids=str)
def test_head_exact_run_stays_below_2_24(shape, C, identity):
    for K in T.HEAD_K:
        o = T.HeadOps(shape, C, K, "exact", None, identity)
        _exact_ok(o)
        if shape == (3, 9, 7) and C == 8:                 # the stored g is the float64 g in both storage types
            g = T.head_ref(o, bounds=False)["g"]
            assert all(torch.equal(g.to(dt).double(), g) for dt in DTS)
            assert bool((o.y * o.scale + o.shift == 0).any()), "no pre-activation is exactly 0: the strict '>' is not exercised"


def test_head_cap_case_stays_below_2_24():
    shape, C, K, _ = T.HEAD_CAP
    gr = _exact_ok(T.HeadOps(shape, C, K, "exact", None, False))
    print(gr)


@pytest.mark.parametrize("dt", DTS, ids=str)
@pytest.mark.parametrize("C", T.HEAD_C)
@pytest.mark.parametrize("shape", T.HEAD_GRID, ids=str)
def test_head_gaussian_seeds_leave_few_relu_decisions_open(shape, C, dt):
    for identity in (False, True):
        share = float(T.head_open(T.HeadOps(shape, C, 1, "gauss", dt, identity)).double().mean())
        assert share <= 1e-4, share


def test_head_cases_have_their_edges():
    from stfunet import _lib
    lib = _lib.load()
    for N, H, W in T.HEAD_GRID + [T.HEAD_PIXEL[0], T.HEAD_CAP[0]]:
        for C in T.HEAD_C:
            assert lib.stf_head_tiles(N, H, W, C) == T.head_tiles(N * H * W, C)
    assert 1 * 1 * 1 * (512 // 8) <= 64                    # one pixel: at most one wave of units
    assert (9 * 7) % 64 and 3 * 9 * 7 * (8 // 8) < T.NT    # image boundaries inside a wave; below one block at C = 8
    assert 2 * 64 * 64 * (512 // 8) > T.HEAD_TILE_CAP * T.NT          # the backward's second grid-stride pass
    (N, H, W), C, _, _ = T.HEAD_CAP
    units, stride = N * H * W * (C // 8), T.HEAD_FWD_CAP * T.NT
    assert units > stride and units % (4 * stride) and units < 2 ** 31


# ------------------------------------------------------------------ MaxPool(3, 2, 1)
@pytest.mark.parametrize("C", T.POOL_C)
@pytest.mark.parametrize("hw", T.POOL_HW, ids=str)
def test_pool_reference(hw, C):
    H, W = hw
    x = T.pool_input(H, W, C)
    dout = T.ri(T._gen("pool_d", hw, C), -8, 8, T.POOL_N, C, T.pool_out(H), T.pool_out(W))
    out, codes, dx, ab = T.pool_ref(x, dout)
    # the codes against an independent first-maximum scan with -inf padding
    o2, c2 = _bn_ref.ref_pool3_fwd(T.nhwc(x), (T.POOL_N, H, W, C, 1))
    assert torch.equal(T.nhwc(out), o2) and torch.equal(T.nhwc(codes), c2)
    assert torch.equal(T.nhwc(dx), _bn_ref.ref_pool3_bwd(c2, T.nhwc(dout), (T.POOL_N, H, W, C, 1), None))
    assert float(out.min()) < 0, "no window of negative values"
    assert bool((ab >= dx.abs()).all())
    if H * W > 1:
        win = F.unfold(F.pad(x, (1, 1, 1, 1), value=-float("inf")), 3, stride=2)      # [N][C*9][L]
        ties = (win.view(T.POOL_N, C, 9, -1) == out.flatten(2).unsqueeze(2)).sum(2)
        assert float((ties > 1).double().mean()) > 0.2, "few ties"


# ------------------------------------------------------------------ bilinear, align_corners=True
@pytest.mark.parametrize("shape", T.RESIZE, ids=str)
def test_resize_reference(shape):
    H, W, h, w = shape
    gen = T._gen("resize_cpu", shape)
    x = (torch.rand((2, H, W, 8), generator=gen) * 2 - 1).float()
    y, ab = T.resize_fwd(x.double(), h, w)
    want = F.interpolate(x.permute(0, 3, 1, 2), size=(h, w), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    assert float((y - want.double()).abs().max()) <= 1e-6
    assert bool((ab >= y.abs() - 1e-12).all())
    # the adjoint: <A x, d> = <x, A^T d>, and float64 autograd of F.interpolate (float64 tables: 1e-6 of the terms)
    d = torch.randn((2, h, w, 8), generator=gen).double()
    dx, dab, cnt = T.resize_bwd(d, H, W)
    assert abs(float((y * d).sum() - (x.double() * dx).sum())) <= 1e-9 * float((y * d).abs().sum() + 1)
    xr = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    F.interpolate(xr, size=(h, w), mode="bilinear", align_corners=True).backward(d.permute(0, 3, 1, 2))
    assert bool(((dx - xr.grad.permute(0, 2, 3, 1)).abs() <= 1e-6 * (dab + 1)).all())
    assert cnt.shape == (H, W) and int(cnt.sum()) >= h * w


@pytest.mark.parametrize("shape", sorted(T.RESIZE_DYADIC), ids=str)
def test_resize_exact_shapes_are_exact(shape):
    """Every lambda of these shapes is 0 or 0.5, and the dyadic operands keep forward, backward and the three-frame
    sum representable in both storage types: the GPU test may ask for equality."""
    H, W, h, w = shape
    for n_in, n_out in ((H, h), (W, w)):
        l1 = T.ac_table(n_in, n_out)[3]
        assert set(l1.tolist()) <= {0.0, 0.5}
    x = T.resize_input(shape, "exact", None, "x", 2, H, W, 8)
    d = T.resize_input(shape, "exact", None, "dy", 2, h, w, 8)
    y, dx = T.resize_fwd(x, h, w)[0], T.resize_bwd(d, H, W)[0]
    for dt in DTS:
        assert torch.equal(y.to(dt).double(), y) and torch.equal(dx.to(dt).double(), dx)
    assert torch.equal((3 * dx + 7).float().double(), 3 * dx + 7)


def test_resize_shapes_have_their_edges():
    assert T.RESIZE_DYADIC <= set(T.RESIZE)
    assert any(max(H / h, W / w) > 20 for H, W, h, w in T.RESIZE) and any(max(h / H, w / W) > 20 for H, W, h, w in T.RESIZE)
    assert any(1 in (H, W) and 1 in (h, w) for H, W, h, w in T.RESIZE)


# ------------------------------------------------------------------ packs
@pytest.mark.parametrize("dt", DTS, ids=str)
def test_pack_values_hold_the_hard_roundings(dt):
    v = T.pack_values(dt, 4096, 0)
    r = v.to(dt)
    assert v.dtype == torch.float32 and bool(torch.isnan(v).any()) and bool(torch.isinf(v).any())
    assert bool(((v == 0) & torch.signbit(v)).any()) and bool(((v == 0) & ~torch.signbit(v)).any())
    fin = torch.isfinite(v)
    lo, hi = torch.nextafter(r, torch.tensor(-float("inf"), dtype=dt)), torch.nextafter(r, torch.tensor(float("inf"), dtype=dt))
    tie = fin & torch.isfinite(r) & (((v - lo.float()) == (hi.float() - v)) | ((v - r.float()).abs() * 2 == (hi.float() - r.float()).abs()))
    assert int(tie.sum()) > 50, "few exact ties"
    tiny = 2.0 ** -14 if dt is torch.float16 else 2.0 ** -126
    assert bool((fin & (r != 0) & (r.float().abs() < tiny)).any()), "no 16-bit subnormal result"
    assert bool((fin & (v != 0) & (r == 0)).any()), "nothing rounds to zero"
    assert bool((fin & torch.isinf(r)).any()), "nothing overflows"


def test_pack_references():
    x = torch.arange(2 * 3 * 2 * 2, dtype=torch.float32).view(2, 3, 2, 2)
    out = T.pack_input_ref(x, 8, torch.bfloat16)
    assert out.shape == (8, 8) and float(out[5, 1]) == float(x[1, 1, 0, 1]) and bool((out[:, 3:] == 0).all())
    B, T_, P, H, W = 2, 3, 3, 2, 2
    s = torch.arange(B * (T_ + P) * H * W, dtype=torch.float32).view(B, T_ + P, 1, H, W)
    out = T.pack_sequence_ref(s, T_, P, 8, torch.float16).view(T_, B, H, W, 8)
    for t in range(T_):
        for b in range(B):
            assert torch.equal(out[t, b, ..., 0].float(), s[b, t, 0])
            for p in range(P):
                assert torch.equal(out[t, b, ..., 1 + p].float(), s[b, T_ + p, 0])
    assert bool((out[..., 1 + P:] == 0).all())
    nan = torch.tensor([float("nan"), 1.0]).to(torch.bfloat16)
    assert T.same16(nan, nan.clone()) and not T.same16(nan, nan.flip(0))


# ------------------------------------------------------------------ channel_sum / stat_sums
def test_channel_sum_and_stat_sums_arguments():
    from stfunet import _lib
    fake = ctypes.c_void_p(1 << 20)                        # fake non-null pointers: nothing runs
    for dt in DTS:
        lib = _lib.load(dt)
        assert lib.stf_channel_sum(fake, 24, 16, 24, fake, fake, None) == T.EINVAL      # C / 8 = 3 does not divide 256
        assert lib.stf_channel_sum(fake, 20, 16, 16, fake, fake, None) == T.EINVAL      # stride not a multiple of 8
        assert lib.stf_stat_sums(fake, 4, 16, 8, 9, fake, None) == T.EINVAL             # c0 + C > Nout
        assert lib.stf_stat_sums(fake, 0, 16, 0, 16, fake, None) == T.EINVAL
        assert lib.stf_stat_sums(None, 4, 16, 0, 16, fake, None) == T.EINVAL


def test_channel_sum_cases_have_their_edges():
    assert max(T.CSUM_M) * 8 < LIMIT                       # |x| <= 8: every sum is exact
    assert T.csum_tiles(70000, 64) == 1024 and 70000 * 8 > 1024 * T.NT
    assert T.csum_tiles(1, 8) == 1 and 257 * 1 > T.NT
    L = T.FOLD_LANES
    assert {1, L - 1, L, L + 1, 4 * L - 1, 4 * L, 4 * L + 1} <= set(T.STAT_TILES)
    assert any(c0 > 0 and C % 16 for _, c0, C in T.STAT_COLS) and all(c0 + C <= n for n, c0, C in T.STAT_COLS)
