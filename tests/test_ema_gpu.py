"""Weight EMA on the device: stf_ema_update / stf_ema_swap against the float64 reference of
_ema_ref.py (exact where fp32 is exact, inside ema_bound elsewhere, bits for the copy, the no-op and
the swap, canaries around every segment on both sides), and stfunet.WeightEMA on real training steps
(shadow against the reference after every update, swap-in evaluation bit for bit against a second
model loaded from the shadow, the step after a swap bit for bit against a run that never swapped).

Largest err/bound seen on an MI355X (printed by the bound tests): 0.988 at the kernel
level (the 8.4 M-element segment at decay 0.999; 0.985 at 0.9), 0.986 over three training steps of
UNet(8, 2, 8).  The final rounding alone reaches 1 / 1.01 of the bound when the result sits just above
a power of two, so figures near 0.99 are what a correct kernel shows on enough elements."""
import copy

import numpy as np
import pytest
import torch

import _ema_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CH = 4096            # ema.hip: EM_CH, elements per chunk
GRID = 2048          # ema.hip: EM_ROWS, the most workgroups
CANARY = 12345.678


@pytest.fixture(scope="module", autouse=True)
def _release_module_state():
    """The module's shared cases (about 0.5 GB of device tensors) and its dead models (a model and
    its program reference each other, so only a collection frees them) go when the module ends:
    nothing of it is resident, or waiting for a collection, while later modules measure memory."""
    yield
    import gc
    _CASES.clear()
    _STATE.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _i32(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_i32(a), _i32(b))


class Case:
    """A table of segments ``(length, odd)``: the model side in one arena with at least four canary
    elements before, between and after the segments (``odd``: the segment starts at an element offset
    that is 1 mod 4, a view only 4-byte aligned), the shadow side at 4-aligned offsets with padding,
    extra gaps and canaries at both ends."""

    def __init__(self, segs, empty_at=None):
        from stfunet.ema import _Table
        self.lens = [n for n, _ in segs]
        mpos, spos, mo, so = [], [], 4, 4
        for i, (n, odd) in enumerate(segs):
            mo = ((mo + 3) & ~3) + (1 if odd else 0)
            mpos.append(mo)
            mo += n + 4
            spos.append(so)
            so += ((n + 3) & ~3) + (4 if i % 2 else 0)
        self.mn, self.sn = ((mo + 3) & ~3) + 4, so + 4
        self.n = sum(self.lens)
        self.midx = torch.cat([torch.arange(o, o + n, device=DEV) for o, n in zip(mpos, self.lens)])
        self.sidx = torch.cat([torch.arange(o, o + n, device=DEV) for o, n in zip(spos, self.lens)])
        self.arena = torch.empty(self.mn, dtype=torch.float32, device=DEV)
        self.shadow = torch.empty(self.sn, dtype=torch.float32, device=DEV)
        assert self.arena.data_ptr() % 16 == 0 and self.shadow.data_ptr() % 16 == 0
        base = self.arena.data_ptr()
        rows = [(base + 4 * o, s, n) for o, s, n in zip(mpos, spos, self.lens)]
        if empty_at is not None:                       # a segment of length 0 with a null model: skipped
            rows.insert(empty_at, (None, 0, 0))
        self.table = _Table(rows, DEV)
        self.odd = [o % 4 for o in mpos]

    def fill(self, e, p):
        self.arena.fill_(CANARY)
        self.shadow.fill_(CANARY)
        self.arena[self.midx] = p
        self.shadow[self.sidx] = e
        self.arena0, self.shadow0 = self.arena.clone(), self.shadow.clone()

    def update(self, w):
        from stfunet._lib import call, stream
        call("stf_ema_update", self.shadow.data_ptr(), self.table.dptr, self.table.hptr, self.table.count, float(w),
             stream())

    def swap(self):
        from stfunet._lib import call, stream
        call("stf_ema_swap", self.shadow.data_ptr(), self.table.dptr, self.table.hptr, self.table.count, stream())

    def check_canaries(self, model_written=False):
        """Everything outside the segments is as it was, on both sides; the model side as a whole
        unless the call writes it."""
        keep = torch.ones(self.sn, dtype=torch.bool, device=DEV)
        keep[self.sidx] = False
        assert _same_bits(self.shadow[keep], self.shadow0[keep]), "shadow outside the segments"
        if model_written:
            keep = torch.ones(self.mn, dtype=torch.bool, device=DEV)
            keep[self.midx] = False
            assert _same_bits(self.arena[keep], self.arena0[keep]), "model outside the segments"
        else:
            assert _same_bits(self.arena, self.arena0), "the update wrote the model"

    def run(self, e, p, w):
        """The shadow's segment elements after one update with weight ``w``; canaries checked."""
        self.fill(e, p)
        self.update(w)
        self.check_canaries()
        return self.shadow[self.sidx]


LENGTHS = [1, 3, 4, 5, CH - 1, CH, CH + 1]
SHAPES = {f"len{n}": dict(segs=[(n, False)]) for n in LENGTHS}
SHAPES["mixed"] = dict(segs=[(1, False), (3, True), (4, False), (5, True), (CH - 1, False), (CH, False),
                             (CH + 1, True)], empty_at=3)
SHAPES["300x64"] = dict(segs=[(64, False)] * 300)
SHAPES["long"] = dict(segs=[(GRID * CH + CH + 5, False)])            # workgroup 0 walks three chunks, 1.. two
SHAPES["odd_view"] = dict(segs=[(2 * CH + 7, True)])
_CASES = {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = Case(**SHAPES[name])
    return _CASES[name]


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


@pytest.mark.parametrize("name", list(SHAPES))
def test_update_is_exact_where_fp32_is(name):
    c = _case(name)
    g = _gen(1)
    e, p = ref.eighths(c.n, g, DEV), ref.eighths(c.n, g, DEV)
    for decay in (0.5, 0.75, 0.875):
        w = np.float32(1.0 - decay)
        got = c.run(e, p, w)
        assert torch.equal(got.double(), ref.ema_step(e, p, w)), decay


@pytest.mark.parametrize("name", list(SHAPES))
def test_update_is_inside_the_bound(name):
    c = _case(name)
    g = _gen(2)
    e, p = ref.log_gaussians(c.n, g, DEV), ref.log_gaussians(c.n, g, DEV)
    for decay in (0.9, 0.999):
        w = np.float32(1.0 - decay)
        got = c.run(e, p, w)
        ratio = float(((got.double() - ref.ema_step(e, p, w)).abs() / ref.ema_bound(e, p, w)).max())
        print(f"{name} decay {decay}: largest err/bound {ratio:.3f}")
        assert ratio <= 1.0, (decay, ratio)


@pytest.mark.parametrize("name", list(SHAPES))
def test_copy_noop_and_nonfinite(name):
    c = _case(name)
    g = _gen(3)
    e, p = ref.log_gaussians(c.n, g, DEV), ref.log_gaussians(c.n, g, DEV)
    p[0] = -0.0
    # w = 1: the model's bits
    assert _same_bits(c.run(e, p, 1.0), p)
    # one inf and one NaN in the model reach only their own elements
    q = p.clone()
    q[0] = float("inf")
    if c.n > 1:
        q[c.n - 1] = float("nan")
    w = np.float32(0.1)
    got = c.run(e, q, w)
    assert got[0] == float("inf") and (c.n == 1 or torch.isnan(got[c.n - 1]))
    mid = slice(1, max(c.n - 1, 1))
    assert torch.isfinite(got[mid]).all()
    assert ((got[mid].double() - ref.ema_step(e[mid], q[mid], w)).abs() <= ref.ema_bound(e[mid], q[mid], w)).all()
    # w = 0: the shadow's bits, whatever the model holds (0 * inf would be a NaN)
    c.fill(e, q)
    c.update(0.0)
    assert _same_bits(c.shadow, c.shadow0) and _same_bits(c.arena, c.arena0)


@pytest.mark.parametrize("name", list(SHAPES))
def test_swap_exchanges_raw_bits(name):
    c = _case(name)
    g = _gen(4)
    e, p = ref.log_gaussians(c.n, g, DEV), ref.log_gaussians(c.n, g, DEV)
    e[0] = -0.0
    _i32(p)[c.n - 1:] = 0x7FC01234                           # a NaN with a payload
    if c.n > 2:
        p[1] = -0.0
        _i32(e)[c.n - 2:c.n - 1] = -4194219                  # 0xFFC00055: sign set, another payload
    c.fill(e, p)
    c.swap()
    c.check_canaries(model_written=True)
    assert _same_bits(c.arena[c.midx], e) and _same_bits(c.shadow[c.sidx], p)
    c.swap()
    assert _same_bits(c.arena, c.arena0) and _same_bits(c.shadow, c.shadow0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_both_libraries_carry_the_same_kernels(dtype):
    from stfunet import _lib
    c = _case("mixed")
    g = _gen(5)
    e, p = ref.log_gaussians(c.n, g, DEV), ref.log_gaussians(c.n, g, DEV)
    w = np.float32(0.001)
    want = c.run(e, p, w).clone()
    with _lib.storage(dtype):
        assert _same_bits(c.run(e, p, w), want)


# ------------------------------------------------------------------ module level
_STATE = {}


def _batch(seed):
    from stfunet.synthetic import dce_batch
    x, t = dce_batch(2, 8, 32, 32, seed=seed, device=DEV)
    return x.flatten(1, 2), t


def _unet():
    """A fresh UNet(8, 2, 8) on the device, the same weights every time."""
    from stfunet import UNet
    torch.manual_seed(0)
    m = UNet(in_channels=8, num_classes=2, base_c=8)
    if "unet" not in _STATE:
        _STATE["unet"] = copy.deepcopy(m.state_dict())
    m.load_state_dict(_STATE["unet"])
    return m.to(DEV).train()


def _adamw(m):
    from stfunet.optim import AdamW
    return AdamW(m.parameters(), lr=1e-2, weight_decay=1e-4)


def _step(m, opt, seed):
    from stfunet import criterion
    x, t = _batch(seed)
    loss = criterion(m(x), t)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss.detach().clone()


def _float_state(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items() if v.is_floating_point()}


def _state_bits_equal(a, b):
    return list(a) == list(b) and all(_same_bits(a[k], b[k]) if a[k].is_floating_point() else torch.equal(a[k], b[k])
                                      for k in a)


@pytest.mark.parametrize("decay,warmup", [(0.9, False), (0.999, True)])
def test_shadow_follows_the_reference_over_training_steps(decay, warmup):
    from stfunet import WeightEMA
    m = _unet()
    opt = _adamw(m)
    ema = WeightEMA(m, decay=decay, warmup=warmup)
    flat = m.program.flat
    assert ema.shadow.numel() == ema.layout.total and ema.layout.segs[0] == (flat.data.data_ptr(), 0, flat.numel)
    pad = torch.ones(flat.numel, dtype=torch.bool, device=DEV)
    for p, off in zip(flat.params, flat.offsets):
        pad[off:off + p.numel()] = False
    assert int(pad.sum()) > 0
    prev, worst = None, 0.0
    for n in range(3):
        _step(m, opt, 30 + n)
        ema.update()
        assert ema.num_updates == n + 1
        cur, got = _float_state(m), ema.state_dict()["shadow"]
        assert list(got) == list(m.state_dict())
        w = ref.weight32(n, decay, warmup)
        seen_buffers = 0
        for k, v in cur.items():
            if n == 0:
                assert _same_bits(got[k], v), k
                continue
            seen_buffers += "running_" in k
            err = (got[k].double() - ref.ema_step(prev[k], v, w)).abs()
            ratio = float((err / ref.ema_bound(prev[k], v, w)).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (k, n, ratio)
        assert n == 0 or seen_buffers > 0
        assert torch.count_nonzero(ema.shadow[:flat.numel][pad]) == 0 and torch.count_nonzero(flat.data[pad]) == 0
        for k, v in m.state_dict().items():                    # integer buffers: the model's own
            if not v.is_floating_point():
                assert torch.equal(got[k], v), k
        prev = {k: v for k, v in got.items() if v.is_floating_point()}
    print(f"UNet(8, 2, 8) decay {decay} warmup {warmup}: largest err/bound {worst:.3f}")


def test_averaged_evaluates_the_shadow_and_leaves_training_untouched():
    """Inside averaged() the model IS a second model loaded from the shadow, bit for bit; after it the
    model's state and its next training step (loss and parameters) are those of a run that never
    swapped: plan replay and packed weights are unaffected."""
    from stfunet import UNet, WeightEMA
    a, b = _unet(), _unet()
    oa, ob = _adamw(a), _adamw(b)
    ema = WeightEMA(a, decay=0.5)
    for n in range(3):
        la, lb = _step(a, oa, 40 + n), _step(b, ob, 40 + n)
        ema.update()
        assert torch.equal(la, lb)
    x, _ = _batch(50)
    second = UNet(in_channels=8, num_classes=2, base_c=8).to(DEV)
    second.load_state_dict(ema.state_dict()["shadow"], strict=True)
    second.eval()
    before = {k: v.detach().clone() for k, v in a.state_dict().items()}
    with torch.no_grad():
        own = a.eval()(x)["out"].clone()
        a.train()
        with ema.averaged() as inside:
            assert inside is a
            a.eval()
            got = a(x)["out"].clone()
            with pytest.raises(RuntimeError, match="swapped"):
                ema.update()
            assert _state_bits_equal({k: v for k, v in a.state_dict().items()},
                                     {k: v for k, v in second.state_dict().items()})
            a.train()
        want = second(x)["out"]
    assert _same_bits(got, want) and not torch.equal(got, own)
    assert ema.num_updates == 3
    assert _state_bits_equal(dict(a.state_dict()), before)
    la, lb = _step(a, oa, 60), _step(b, ob, 60)
    assert _same_bits(la, lb)
    assert _state_bits_equal(dict(a.state_dict()), dict(b.state_dict()))


def test_averaged_swaps_back_when_the_block_raises():
    from stfunet import WeightEMA
    m = _unet()
    ema = WeightEMA(m, decay=0.5)
    ema.update()
    with torch.no_grad():
        for p in m.parameters():
            p.add_(1.0)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    with pytest.raises(KeyError):
        with ema.averaged():
            assert not _state_bits_equal(dict(m.state_dict()), before)
            raise KeyError("inside")
    assert _state_bits_equal(dict(m.state_dict()), before)
    ema.update()                                              # not left swapped


def test_state_dict_round_trip_and_copy_to():
    from stfunet import WeightEMA
    m = _unet()
    opt = _adamw(m)
    ema = WeightEMA(m, decay=0.9, warmup=True)
    for n in range(2):
        _step(m, opt, 70 + n)
        ema.update()
    sd = ema.state_dict()
    assert set(sd) == {"decay", "warmup", "num_updates", "shadow"} and sd["num_updates"] == 2
    fresh = WeightEMA(m, decay=0.5)
    fresh.load_state_dict(sd)
    assert (fresh.decay, fresh.warmup, fresh.num_updates) == (0.9, True, 2)
    assert _same_bits(fresh.shadow, ema.shadow)
    _step(m, opt, 72)
    ema.update()
    fresh.update()
    assert _same_bits(fresh.shadow, ema.shadow) and fresh.num_updates == 3
    first = next(iter(sd["shadow"]))                          # clones: an earlier state dict is not a view
    assert not torch.equal(sd["shadow"][first], ema.state_dict()["shadow"][first])
    other = _unet()
    shadow = ema.shadow.clone()
    ema.copy_to(other)
    assert _state_bits_equal(dict(other.state_dict()), ema.state_dict()["shadow"])
    assert _same_bits(ema.shadow, shadow)


def test_buffers_false_leaves_the_buffers_with_the_model():
    from stfunet import WeightEMA
    m = _unet()
    opt = _adamw(m)
    ema = WeightEMA(m, decay=0.5, buffers=False)
    assert ema.shadow.numel() == m.program.flat.numel and len(ema.layout.segs) == 1
    for n in range(2):
        _step(m, opt, 80 + n)
        ema.update()
    bufs = {k: v.detach().clone() for k, v in m.named_buffers()}
    params = {k: v.detach().clone() for k, v in m.named_parameters()}
    with ema.averaged():
        assert all(_same_bits(v, bufs[k]) if v.is_floating_point() else torch.equal(v, bufs[k])
                   for k, v in m.named_buffers())
        assert any(not torch.equal(v, params[k]) for k, v in m.named_parameters())
    got = ema.state_dict()["shadow"]
    assert list(got) == list(m.state_dict()) and all(torch.equal(got[k], bufs[k]) for k in bufs)


def test_plain_module_parameters_are_segments_of_their_own():
    """Any other nn.Module on the device: one segment per fp32 parameter and float buffer; anything
    else is refused."""
    from stfunet import WeightEMA
    torch.manual_seed(1)
    m = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.BatchNorm1d(5), torch.nn.Linear(5, 3)).to(DEV)
    ema = WeightEMA(m, decay=0.75)
    assert len(ema.layout.segs) == 6 + 2
    ema.update()
    prev = ema.state_dict()["shadow"]
    with torch.no_grad():
        for t in list(m.parameters()) + [m[1].running_mean, m[1].running_var]:
            t.add_(torch.randn_like(t))
    ema.update()
    got = ema.state_dict()["shadow"]
    w = ref.weight32(1, 0.75)
    for k, v in m.state_dict().items():
        if v.is_floating_point():
            assert ((got[k].double() - ref.ema_step(prev[k], v, w)).abs() <= ref.ema_bound(prev[k], v, w)).all(), k
    with pytest.raises(ValueError, match="fp32"):
        WeightEMA(torch.nn.Linear(4, 4).to(DEV).half())


def test_stf_model_one_step_update_and_averaged_forward():
    from stfunet import STFLSTMUNet, WeightEMA, criterion
    from stfunet.synthetic import dce_batch
    torch.manual_seed(0)
    m = STFLSTMUNet(time_steps=4).to(DEV).train()
    opt = _adamw(m)
    ema = WeightEMA(m)
    x, t = dce_batch(1, 4, 64, 64, seed=90, device=DEV, mask_hw=(32, 32))
    loss = criterion(m(x), t)
    opt.zero_grad()
    loss.backward()
    opt.step()
    ema.update()
    keys = list(ema.state_dict()["shadow"])
    assert keys == list(m.state_dict()) and len(keys) == 296
    with torch.no_grad(), ema.averaged():
        m.eval()
        out = m(x)["out"]
        m.train()
    assert torch.isfinite(out).all()


def test_engine_train_one_epoch_and_evaluate_with_the_average():
    from stfunet import UNet, WeightEMA, engine
    m = _unet()
    opt = _adamw(m)
    ema = WeightEMA(m, decay=0.5)
    batches = [_batch(s) for s in (21, 22)]
    loader = [(x.view(2, 8, 1, 32, 32), t) for x, t in batches]       # preprocess_input flattens
    sch = engine.create_lr_scheduler(opt, 2, 1)
    engine.train_one_epoch(m, opt, loader, torch.device(DEV), 0, 2, lr_scheduler=sch, print_freq=1, ema=ema)
    assert ema.num_updates == 2
    second = UNet(in_channels=8, num_classes=2, base_c=8).to(DEV)
    second.load_state_dict(ema.state_dict()["shadow"], strict=True)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    got = engine.evaluate(m, loader, torch.device(DEV), 2, ema=ema)
    want = engine.evaluate(second, loader, torch.device(DEV), 2)
    own = engine.evaluate(m, loader, torch.device(DEV), 2)
    assert got["dice"] == want["dice"]
    assert torch.equal(got["confusion_matrix"].mat, want["confusion_matrix"].mat)
    assert int(own["confusion_matrix"].mat.sum()) == int(got["confusion_matrix"].mat.sum())
    assert _state_bits_equal(dict(m.state_dict()), before)
    ck = engine.checkpoint_dict(m, opt, sch, 0, {}, ema=ema)
    fresh = WeightEMA(m, decay=0.9)
    assert engine.resume_from(ck, m, opt, sch, ema=fresh) == 1
    assert fresh.num_updates == 2 and fresh.decay == 0.5 and _same_bits(fresh.shadow, ema.shadow)
