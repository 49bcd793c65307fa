"""Gradient clipping by the global L2 norm on the GPU: the three entry points against float64
restatements on the host, then ``stfunet.optim.clip_grad_norm_``, ``AdamW(max_grad_norm=...)`` and
``engine.train_one_epoch(..., max_grad_norm=...)`` on small models after a real backward.

Bounds.  ``stf_grad_norm`` squares and sums in double: the sum's relative error is below
n * 2^-53 (n <= 2^24 here: 2^-29), the square root halves it, so the fp32 result is within 1 fp32
ulp of the fp32 rounding of the float64 norm (at most the neighbour when the exact value sits on
a rounding boundary).  Everything else about the kernels is compared bit for bit.

What "bit for bit" is compared with.  ``stf_adamw_clip`` shares the kernel body of
``stf_adamw_dev`` (the device-scalar update of ``capturable=True`` and of the GradScaler step), so
the fused step is compared bitwise with ``clip_grad_norm_`` followed by the unclipped step that runs
that body, ``AdamW(capturable=True).step()``.  The default host-scalar step runs ``stf_adamw``, a
different kernel that has never had ``stf_adamw_dev``'s last bits, clipping or not: its bias
corrections come from the fp64 betas (1 - 0.999 ** step) where the device kernels raise the betas
rounded to fp32 (1 - fl32(0.999) ** step, 1.29e-5 away at step 1), and its second moment is one fma
where theirs is a product and a sum.  Against that step the first moment is compared bitwise, the
second to a few ulps, and the parameters to the bound ``_host_scalar_bound`` derives from those two
roundings (7.2e-6 at step 1; measured on an MI355X: 6.75e-6 to 6.78e-6, the same with the clip active
and with the coefficient at exactly 1).
"""
import contextlib
import copy
import os

import numpy as np
import pytest
import torch

import _launch_trace as lt

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
NAN, BIG = float("nan"), 1e30


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.int32)


def _ulps(a, b):
    """Distance in fp32 ulps between two positive finite fp32 numbers."""
    return abs(int(_bits(a).reshape(-1)[0]) - int(_bits(b).reshape(-1)[0]))


def _coef(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient, in fp32."""
    c = F32(max_norm) / (F32(norm) + F32(1e-6))
    return F32(1.0) if c > F32(1.0) else c


# ------------------------------------------------------------------ kernel harness
class _Case:
    """Segments of the given lengths in one buffer: 8 elements in front, the padding to a multiple
    of 4 plus (every other segment) 4 more elements between segments and 8 behind, all of them
    prefilled with NaN and 1e30 alternately; the segments hold N(0, 1) values."""

    def __init__(self, lens, seed=0):
        from stfunet.optim import _SegTable
        rng = np.random.default_rng(seed)
        segs, off = [], 8
        for i, n in enumerate(lens):
            segs.append((off, n))
            off += ((n + 3) & ~3) + (4 if i % 2 else 0)
        total = off + 8
        host = np.empty(total, dtype=F32)
        host[0::2], host[1::2] = NAN, BIG
        self.inside = np.zeros(total, dtype=bool)
        for o, n in segs:
            host[o:o + n] = rng.standard_normal(n).astype(F32)
            self.inside[o:o + n] = True
        self.host, self.segs = host, segs
        self.table = _SegTable(segs, DEV)
        self.norm64 = float(np.sqrt(np.sum(host[self.inside].astype(np.float64) ** 2)))

    def device(self, values=None):
        return torch.from_numpy(self.host if values is None else values).to(DEV)


LENS = {
    "n1": [1], "n3": [3], "n4": [4], "n5": [5], "n4095": [4095], "n4096": [4096], "n4097": [4097],
    "n1M": [(1 << 20) + 7],
    "wrap": [2048 * 4096 + 3 * 4096 + 5],            # more chunks than workgroups: the grid wraps
    "t2": [4097, 5],
    "t37": [2 * ((131 * i) % 3000) + 1 for i in range(36)] + [40001],
}
_CASES = {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = _Case(LENS[name], seed=len(_CASES))
    return _CASES[name]


def _norm(buf, table, max_norm, scale=None):
    """(out[4], partial rows) of one stf_grad_norm, on the host."""
    from stfunet._lib import call, stream
    from stfunet.nhwc import _p
    out = torch.full((4,), 7.0, device=DEV)
    table.partial.fill_(-1.0)
    call("stf_grad_norm", _p(buf), _p(table.dev), table.hptr, table.count, _p(scale), float(max_norm),
         _p(table.partial), _p(out), stream())
    return out.cpu().numpy(), table.partial.cpu().numpy().copy(), out


def _scale(buf, table, out):
    from stfunet._lib import call, stream
    from stfunet.nhwc import _p
    call("stf_grad_scale", _p(buf), _p(table.dev), table.hptr, table.count, _p(out), stream())


@pytest.mark.parametrize("name", list(LENS))
def test_norm_coefficient_and_determinism(name):
    """Norm within 1 ulp of the fp32 rounding of the float64 norm although every gap holds NaN / 1e30;
    coefficient = torch's fp32 expression of the kernel's own norm, exactly 1 below max_norm; two runs
    give the same bits in out and in the partial rows."""
    c = _case(name)
    buf = c.device()
    want = F32(c.norm64)
    lo, hi = 0.37 * c.norm64, 2.0 * c.norm64
    out, rows, _ = _norm(buf, c.table, lo)
    print(f"{name}: norm {out[0]!r} float64 {c.norm64!r} ulps {_ulps(out[0], want)} rows {len(rows)}")
    assert np.isfinite(out[0]) and _ulps(out[0], want) <= 1
    assert out[2] == 0.0 and out[3] == 0.0
    assert _bits(out[1]) == _bits(_coef(out[0], lo)) and out[1] < 1.0
    assert len(rows) == c.table.partial.numel() and np.all(rows >= 0.0)       # every row written
    out2, rows2, _ = _norm(buf, c.table, lo)
    assert np.array_equal(_bits(out), _bits(out2)) and np.array_equal(rows.view(np.int64), rows2.view(np.int64))
    out3, _, _ = _norm(buf, c.table, hi)
    assert out3[1] == 1.0 and _bits(out3[0]) == _bits(out[0])
    assert torch.equal(buf.cpu().view(torch.int32), torch.from_numpy(c.host).view(torch.int32))   # read only


@pytest.mark.parametrize("name", list(LENS))
def test_scale_in_segments_only(name):
    """After stf_grad_scale every in-segment element is g * coef (fp32, bit for bit) and every other
    byte is as it was; with a coefficient of exactly 1 the whole buffer keeps its bits."""
    c = _case(name)
    buf = c.device()
    out, _, dev_out = _norm(buf, c.table, 0.37 * c.norm64)
    _scale(buf, c.table, dev_out)
    got = buf.cpu().numpy()
    want = c.host.copy()
    want[c.inside] = c.host[c.inside] * F32(out[1])
    assert np.array_equal(_bits(got), _bits(want))
    buf = c.device()
    _, _, dev_out = _norm(buf, c.table, 2.0 * c.norm64)
    _scale(buf, c.table, dev_out)
    assert np.array_equal(_bits(buf.cpu().numpy()), _bits(c.host))


@pytest.mark.parametrize("name", ["n4097", "t37"])
@pytest.mark.parametrize("value", [1e20, 1e-30])
def test_norm_range(name, value):
    """All elements 1e20 (squares overflow fp32) and all 1e-30 (squares flush to 0 in fp32): the norm
    is finite, non-zero and right."""
    c = _case(name)
    host = c.host.copy()
    host[c.inside] = F32(value)
    n = int(c.inside.sum())
    want = F32(np.sqrt(float(n)) * float(F32(value)))
    out, _, _ = _norm(c.device(host), c.table, 1.0)
    print(f"{name} {value}: norm {out[0]!r} want {want!r}")
    assert np.isfinite(out[0]) and out[0] > 0 and _ulps(out[0], want) <= 1 and out[2] == 0.0


@pytest.mark.parametrize("name", ["n5", "n4097", "t37"])
@pytest.mark.parametrize("bad", [float("inf"), NAN])
def test_nonfinite_in_the_scalar_tail_sets_the_flag(name, bad):
    c = _case(name)
    o, n = c.segs[-1]
    assert n % 4                                   # the last element is in the scalar tail
    host = c.host.copy()
    host[o + n - 1] = bad
    out, _, _ = _norm(c.device(host), c.table, 1.0)
    assert out[2] == 1.0 and not np.isfinite(out[0]) and out[3] == 0.0
    out, _, _ = _norm(c.device(), c.table, 1.0)
    assert out[2] == 0.0


@pytest.mark.parametrize("name", ["n4097", "t37", "n1M"])
def test_grad_scale_argument(name):
    """A buffer that carries a 65536 loss scale, with grad_scale = 65536: the norm of the unscaled
    buffer (within 1 ulp of the run on the pre-divided buffer)."""
    c = _case(name)
    plain, _, _ = _norm(c.device(), c.table, 1.0)
    scaled = c.host.copy()
    scaled[c.inside] *= F32(65536.0)
    s = torch.full((1,), 65536.0, device=DEV)
    out, _, _ = _norm(c.device(scaled), c.table, 1.0, s)
    assert _ulps(out[0], plain[0]) <= 1 and out[2] == 0.0
    assert _bits(out[1]) == _bits(_coef(out[0], 1.0))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_both_libraries_carry_the_same_kernels(dtype):
    from stfunet import _lib
    c = _case("t37")
    ref, ref_rows, _ = _norm(c.device(), c.table, 1.0)
    with _lib.storage(dtype):
        out, rows, _ = _norm(c.device(), c.table, 1.0)
    assert np.array_equal(_bits(out), _bits(ref)) and np.array_equal(rows, ref_rows)


def _adamw_state(n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda s=1.0: torch.randn(n, device=DEV, generator=g) * s          # noqa: E731
    return r(), r(), r(0.1), r(0.1).abs()


def _adamw_dev(p, g, m, v, hyper):
    from stfunet._lib import call, stream
    from stfunet.nhwc import _p
    call("stf_adamw_dev", _p(p), _p(g), _p(m), _p(v), p.numel(), _p(hyper), 0.9, 0.999, 1e-8, 1e-2, stream())


def _adamw_clip(p, g, m, v, hyper, clip, scale=None, finf=None):
    from stfunet._lib import call, stream
    from stfunet.nhwc import _p
    call("stf_adamw_clip", _p(p), _p(g), _p(m), _p(v), p.numel(), _p(hyper), _p(scale), _p(finf), _p(clip),
         0.9, 0.999, 1e-8, 1e-2, stream())


def test_adamw_clip_against_adamw_dev():
    """Coefficient 1, no scale: the bits of stf_adamw_dev.  Coefficient 0.25 with scale 1024: the bits
    of stf_adamw_dev fed (g * (1/1024)) * 0.25 computed in fp32 on the host in that order.  The step
    count advances on the device; the gradient is not modified."""
    n = 10007
    p0, g, m0, v0 = _adamw_state(n, 3)
    for coef, scale in ((1.0, None), (0.25, 1024.0)):
        pa, ma, va = p0.clone(), m0.clone(), v0.clone()
        pb, mb, vb = p0.clone(), m0.clone(), v0.clone()
        gh = g.cpu().numpy()
        if scale is not None:
            gh = gh * (F32(1.0) / F32(scale))
        gh = gh * F32(coef)
        _adamw_dev(pa, torch.from_numpy(gh).to(DEV), ma, va, torch.tensor([1e-2, 3.0], device=DEV))
        hyper = torch.tensor([1e-2, 2.0], device=DEV)           # the clipped entry point increments it
        clip = torch.tensor([123.0, coef, 0.0, 0.0], device=DEV)
        sc = None if scale is None else torch.full((1,), scale, device=DEV)
        gb = g.clone()
        _adamw_clip(pb, gb, mb, vb, hyper, clip, sc)
        assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)
        assert hyper[1].item() == 3.0 and torch.equal(gb, g)
        assert not torch.equal(pb, p0)


@pytest.mark.parametrize("why", ["norm", "found_inf"])
def test_adamw_clip_skips(why):
    """out[2] = 1 or found_inf = 1: parameters, moments and hyper[1] keep their bits."""
    p0, g, m0, v0 = _adamw_state(4099, 4)
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    hyper = torch.tensor([1e-2, 5.0], device=DEV)
    clip = torch.tensor([float("inf") if why == "norm" else 1.0, 0.5, 1.0 if why == "norm" else 0.0, 0.0], device=DEV)
    finf = torch.tensor([0.0 if why == "norm" else 1.0], device=DEV)
    _adamw_clip(p, g, m, v, hyper, clip, None, finf)
    assert torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(v, v0) and hyper[1].item() == 5.0
    clip[2] = 0.0
    finf.zero_()
    _adamw_clip(p, g, m, v, hyper, clip, None, finf)
    assert hyper[1].item() == 6.0 and not torch.equal(p, p0)


# ------------------------------------------------------------------ package level
@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


STF_ENC = ("conv1", "bn1", "layer1", "layer2", "layer3", "layer4")
_STATE = {}


def _batch(which, seed=11):
    from stfunet.synthetic import dce_batch
    if which == "unet":
        x, t = dce_batch(2, 8, 32, 32, seed=seed, device=DEV)
        return x.flatten(1, 2), t
    return dce_batch(1, 2, 32, 32, seed=seed, device=DEV, mask_hw=(16, 16))      # logits at half resolution


def _model(which, dtype=torch.bfloat16, freeze=False):
    """A fresh copy (same weights every time) after one real eager backward of the criterion."""
    from stfunet import STFLSTMUNet, UNet
    torch.manual_seed(0)
    m = UNet(in_channels=8, num_classes=2, base_c=8) if which == "unet" else STFLSTMUNet(time_steps=2)
    if which not in _STATE:
        _STATE[which] = copy.deepcopy(m.state_dict())
    m.load_state_dict(_STATE[which])
    m.storage_dtype = dtype
    m = m.to(DEV).train()
    if freeze:
        for n in STF_ENC:
            m.get_submodule(n).requires_grad_(False)
    return m


def _backward(m, which, scale=1.0, seed=11):
    from stfunet import criterion
    x, t = _batch(which, seed)
    with _env(STF_PLAN="0"):
        (criterion(m(x), t) * scale).backward()
    torch.cuda.synchronize()
    return m


def _norm64(grads):
    return float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads)))


def _grads(m):
    return [p.grad for p in m.parameters() if p.grad is not None]


def _moments(opt):
    return [(s["exp_avg"], s["exp_avg_sq"]) for s in (opt.state[p] for g in opt.param_groups for p in g["params"])]


def _host_scalar_bound(step=1, b1=0.9, b2=0.999):
    """Largest relative difference of one update between stf_adamw (bias corrections of the fp64 betas,
    rounded to fp32) and the stf_adamw_dev body (the same of the betas rounded to fp32): the update is
    lr / bc1 * m / (sqrt(v / bc2) + eps), so d(bc1) / bc1 + d(bc2) / (2 bc2), plus 8 fp32 roundings
    (2^-24 each) for the differently contracted second moment and the operations after it.  A
    parameter that starts at 0 is its update, so this bounds the parameters' difference too."""
    h1, h2 = float(F32(1.0 - b1 ** step)), float(F32(1.0 - b2 ** step))
    d1, d2 = float(F32(1.0 - float(F32(b1)) ** step)), float(F32(1.0 - float(F32(b2)) ** step))
    return abs(d1 - h1) / h1 + 0.5 * abs(d2 - h2) / h2 + 8 * 2.0 ** -24


def _step_count(opt):
    return int(opt.state_dict()["state"][0]["step"])


@pytest.mark.parametrize("which", ["unet", "stf"])
def test_clip_grad_norm_on_the_flat_gradients(which):
    from stfunet.optim import _CLIP_TABLES, clip_grad_norm_
    m = _backward(_model(which), which)
    before = [g.clone() for g in _grads(m)]
    want = _norm64(before)
    n = clip_grad_norm_(m, 0.37 * want)                        # a model is accepted
    assert n.dim() == 0 and n.is_cuda
    hit = _CLIP_TABLES[tuple(id(p) for p in m.parameters())]
    assert hit[1] is not None                                  # the in-place path over the flat buffer
    print(f"{which}: norm {n.item()!r} float64 {want!r} segments {hit[1][1].count}")
    assert _ulps(n.item(), F32(want)) <= 1
    coef = torch.tensor(_coef(n.item(), 0.37 * want), device=DEV)
    assert all(torch.equal(g, b * coef) for g, b in zip(_grads(m), before))
    after = [g.clone() for g in _grads(m)]
    n2 = clip_grad_norm_(m.parameters(), 10.0 * want)          # below max_norm: nothing changes
    assert all(torch.equal(g, b) for g, b in zip(_grads(m), after)) and n2.item() < n.item()


def test_clip_grad_norm_on_scattered_parameters():
    from stfunet.optim import clip_grad_norm_
    g = torch.Generator(device=DEV).manual_seed(9)
    ps = [torch.nn.Parameter(torch.zeros(s, device=DEV)) for s in ((5,), (3, 4), (1,), (7, 3))]
    for p in ps:
        p.grad = torch.randn(p.shape, device=DEV, generator=g)
    ps.append(torch.nn.Parameter(torch.zeros(6, device=DEV)))          # no gradient: left out
    before = [p.grad.clone() for p in ps[:-1]]
    want = _norm64(before)
    n = clip_grad_norm_(ps, 0.5 * want)
    assert _ulps(n.item(), F32(want)) <= 1 and ps[-1].grad is None
    coef = torch.tensor(_coef(n.item(), 0.5 * want), device=DEV)
    assert all(torch.equal(p.grad, b * coef) for p, b in zip(ps, before))
    ps[0].grad[0] = float("inf")
    with pytest.raises(RuntimeError, match="non-finite"):
        clip_grad_norm_(ps, 1.0, error_if_nonfinite=True)


@pytest.mark.parametrize("active", [True, False], ids=["clipping", "below"])
@pytest.mark.parametrize("which", ["unet", "stf"])
def test_fused_step_against_unfused(which, active):
    """AdamW(max_grad_norm=m).step() on copy A against clip_grad_norm_ + the unclipped step on copy B
    (same weights, same gradients): parameters and moments bit-identical with the unclipped step that
    runs the shared kernel body (capturable=True), the reported norms equal, .grad of A untouched.
    Copy C takes the default host-scalar step (stf_adamw, another kernel: module docstring): first
    moment bitwise, second moment and parameters to the bound derived from the two kernels' roundings."""
    from stfunet.optim import AdamW, clip_grad_norm_
    a, b, c = (_backward(_model(which), which) for _ in range(3))
    ga = [g.clone() for g in _grads(a)]
    assert all(torch.equal(x, y) for x, y in zip(ga, _grads(b)))
    norm = _norm64(ga)
    mx = (0.37 if active else 3.0) * norm
    kw = dict(lr=1e-2, weight_decay=1e-2)
    oa = AdamW(a.parameters(), max_grad_norm=mx, **kw)
    ob = AdamW(b.parameters(), capturable=True, **kw)
    oc = AdamW(c.parameters(), **kw)
    oa.step()
    nb = clip_grad_norm_(b.parameters(), mx)
    ob.step()
    clip_grad_norm_(c.parameters(), mx)
    oc.step()
    torch.cuda.synchronize()
    assert torch.equal(oa.grad_norm, nb) and _ulps(nb.item(), F32(norm)) <= 1
    assert all(torch.equal(x, y) for x, y in zip(ga, _grads(a)))               # .grad unclipped
    assert (not active) or not torch.equal(_grads(b)[0], ga[0])
    for (n, pa), pb in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(pa, pb), n
    for (ma, va), (mb, vb) in zip(_moments(oa), _moments(ob)):
        assert torch.equal(ma, mb) and torch.equal(va, vb)
    assert _step_count(oa) == 1 and _step_count(ob) == 1
    rel = lambda x, y: ((x.double() - y.double()).norm() / y.double().norm().clamp_min(1e-30)).item()   # noqa: E731
    for (ma, va), (mc, vc) in zip(_moments(oa), _moments(oc)):
        assert torch.equal(ma, mc) and rel(va, vc) < 4 * 2.0 ** -24
    worst = max(rel(pa, pc) for pa, pc in zip(a.parameters(), c.parameters()))
    print(f"{which} active={active}: fused vs host-scalar step, worst parameter rel {worst:.3e} "
          f"(bound {_host_scalar_bound():.3e})")
    assert worst < _host_scalar_bound()


def test_fused_step_against_float64_adamw():
    """The fused step's parameters against AdamW restated here in float64 from gradients clipped in
    float64: the 1e-6 relative bound of tests/test_kernels_gpu.py's stf_adamw test."""
    from stfunet.optim import AdamW
    a = _backward(_model("unet"), "unet")
    lr, wd, b1, b2, eps = 1e-2, 1e-2, 0.9, 0.999, 1e-8
    p0 = [p.detach().double().clone() for p in a.parameters()]
    g64 = [g.double() for g in _grads(a)]
    norm = _norm64(g64)
    mx = 0.37 * norm
    opt = AdamW(a.parameters(), lr=lr, weight_decay=wd, betas=(b1, b2), eps=eps, max_grad_norm=mx)
    opt.step()
    coef = min(1.0, mx / (norm + 1e-6))
    num = den = 0.0
    for p, q, g in zip(a.parameters(), p0, g64):
        g = g * coef
        m, v = (1 - b1) * g, (1 - b2) * g * g
        q = q * (1 - lr * wd) - (lr / (1 - b1)) * m / (v.sqrt() / (1 - b2) ** 0.5 + eps)
        num += float((p.detach().double() - q).pow(2).sum())
        den += float(q.pow(2).sum())
    print(f"fused step vs float64 AdamW: rel {np.sqrt(num / den):.3e}")
    assert np.sqrt(num / den) < 1e-6


def test_launch_trace_of_the_step():
    """Entry points reached through stfunet._lib.call (what the tracing helper of the frozen-step
    test records): without max_grad_norm exactly ["stf_adamw"], with it stf_grad_norm (streaming
    pass + fold) and stf_adamw_clip (step count + update, like stf_adamw_amp)."""
    from stfunet.optim import AdamW
    a, b = _backward(_model("unet"), "unet"), _backward(_model("unet"), "unet")
    oa, ob = AdamW(a.parameters(), lr=1e-3), AdamW(b.parameters(), lr=1e-3, max_grad_norm=1.0)
    with lt.tracing() as trace:
        oa.step()
        torch.cuda.synchronize()
    assert trace == ["stf_adamw"]
    with lt.tracing() as trace:
        ob.step()
        torch.cuda.synchronize()
    assert trace == ["stf_grad_norm", "stf_adamw_clip"]
    fb = ob._flat[0]
    assert fb["p"] is not None and fb["gscratch"] is None          # in place: no gather, no gradient copy
    ob.param_groups[0]["max_grad_norm"] = None                      # the option off again: today's step
    with lt.tracing() as trace:
        ob.step()
        torch.cuda.synchronize()
    assert trace == ["stf_adamw"] and _step_count(ob) == 2


def test_frozen_encoder_slices_and_padding_stay_out():
    """STF with the encoder frozen: NaN written over the frozen parameters' slices of the flat gradient
    buffer and over all padding enters neither form's norm; the step is taken; frozen parameters keep
    their bits."""
    from stfunet.optim import AdamW, clip_grad_norm_
    models = [_backward(_model("stf", freeze=True), "stf") for _ in range(2)]
    for m in models:
        flat = m.program.flat
        for p, off in zip(flat.params, flat.offsets):
            n = p.numel()
            if not p.requires_grad:
                assert p.grad is None
                flat.grad[off:off + n] = NAN
            flat.grad[off + n:off + ((n + 3) & ~3)] = NAN
    a, b = models
    train = [p for p in a.parameters() if p.requires_grad]
    want = _norm64([p.grad for p in train])
    before = {n: p.detach().clone() for n, p in a.named_parameters()}
    opt = AdamW(train, lr=1e-2, max_grad_norm=0.37 * want)
    opt.step()
    nb = clip_grad_norm_([p for p in b.parameters() if p.requires_grad], 0.37 * want)
    nb2 = clip_grad_norm_(b, 0.37 * want)                      # the whole model: frozen .grad is None
    print(f"frozen: fused {opt.grad_norm.item()!r} function {nb.item()!r} float64 {want!r}")
    assert np.isfinite(want) and _ulps(opt.grad_norm.item(), F32(want)) <= 1 and torch.equal(opt.grad_norm, nb)
    assert np.isfinite(nb2.item()) and nb2.item() < nb.item()
    assert _step_count(opt) == 1
    moved = 0
    for n, p in a.named_parameters():
        if p.requires_grad:
            assert torch.isfinite(p).all(), n
            moved += int(not torch.equal(p, before[n]))
        else:
            assert torch.equal(p, before[n]), n
    assert moved > 0


def test_gradscaler_step_without_unscale():
    """fp16 storage, GradScaler(init_scale=65536), no unscale_: grad_norm is the unscaled norm; a step
    with an injected inf is skipped (parameters, moments, count untouched) and the scale halves; the
    next clean step advances the count by one."""
    from stfunet import criterion
    from stfunet.optim import AdamW
    m = _model("unet", torch.float16)
    opt = AdamW(m.parameters(), lr=1e-3, max_grad_norm=1e-3)
    scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)

    def backward(seed):
        x, t = _batch("unet", seed)
        opt.zero_grad()
        with _env(STF_PLAN="0"):
            scaler.scale(criterion(m(x), t)).backward()

    backward(11)
    want = _norm64([g / 65536.0 for g in _grads(m)])
    scaler.step(opt)
    scaler.update()
    print(f"amp: grad_norm {opt.grad_norm.item()!r} float64 of .grad / scale {want!r}")
    assert _ulps(opt.grad_norm.item(), F32(want)) <= 1 and want > 1e-3
    assert _step_count(opt) == 1 and scaler.get_scale() == 65536.0
    backward(12)
    _grads(m)[3].view(-1)[1] = float("inf")
    p0 = [p.detach().clone() for p in m.parameters()]
    s0 = [(a.clone(), b.clone()) for a, b in _moments(opt)]
    scaler.step(opt)
    scaler.update()
    assert scaler.get_scale() == 32768.0 and _step_count(opt) == 1
    assert all(torch.equal(p, q) for p, q in zip(m.parameters(), p0))
    assert all(torch.equal(a, c) and torch.equal(b, d) for (a, b), (c, d) in zip(_moments(opt), s0))
    backward(13)
    scaler.step(opt)
    scaler.update()
    assert _step_count(opt) == 2 and np.isfinite(opt.grad_norm.item())
    assert not all(torch.equal(p, q) for p, q in zip(m.parameters(), p0))


def test_capturable_equals_host_scalar_mode_with_clipping():
    from stfunet.optim import AdamW
    a, b = _backward(_model("unet"), "unet"), _backward(_model("unet"), "unet")
    norm = _norm64(_grads(a))
    oa = AdamW(a.parameters(), lr=1e-2, max_grad_norm=0.37 * norm)
    ob = AdamW(b.parameters(), lr=1e-2, max_grad_norm=0.37 * norm, capturable=True)
    for step in range(3):
        for o in (oa, ob):
            o.param_groups[0]["lr"] = 1e-2 / (step + 1)
            o.step()
        assert torch.equal(oa.grad_norm, ob.grad_norm)
    for (n, pa), pb in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(pa, pb), n
    for (ma, va), (mb, vb) in zip(_moments(oa), _moments(ob)):
        assert torch.equal(ma, mb) and torch.equal(va, vb)
    assert _step_count(oa) == 3 and _step_count(ob) == 3


@pytest.mark.parametrize("max_norm", [1e-3, None])
def test_train_one_epoch(max_norm, capsys):
    """Two synthetic batches through engine.train_one_epoch against the hand-written loop that calls
    the (fused) optimizer directly; None: the loop without clipping, and no grad_norm meter."""
    from stfunet import criterion, engine
    from stfunet.optim import AdamW
    a, b = _model("unet"), _model("unet")
    batches = [_batch("unet", s) for s in (21, 22)]
    loader = [(x.view(2, 8, 1, 32, 32), t) for x, t in batches]       # preprocess_input flattens
    oa = AdamW(a.parameters(), lr=1e-2, weight_decay=1e-4)
    sa = engine.create_lr_scheduler(oa, 2, 1)
    engine.train_one_epoch(a, oa, loader, torch.device(DEV), 0, 2, lr_scheduler=sa, print_freq=1,
                           max_grad_norm=max_norm)
    printed = capsys.readouterr().out
    assert ("grad_norm:" in printed) == (max_norm is not None)
    assert oa.param_groups[0]["max_grad_norm"] is None                # put back after the epoch
    ob = AdamW(b.parameters(), lr=1e-2, weight_decay=1e-4, max_grad_norm=max_norm)
    sb = engine.create_lr_scheduler(ob, 2, 1)
    for x, t in batches:
        loss = criterion(b(x), t)
        ob.zero_grad()
        loss.backward()
        ob.step()
        sb.step()
        if max_norm is not None:
            assert ob.grad_norm.item() > max_norm                     # the clip was active
    for (n, pa), pb in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(pa, pb), n
