"""Weight EMA, the parts that need no GPU: the float64 reference and its bound against torch's own
AveragedModel, the decay schedule, the segment builder, the entry points' argument checks (nothing
is launched) and the public surface."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import _ema_ref as ref

EINVAL = 100001
FAKE = 1 << 20                          # a non-null, 16-byte aligned "device" address: nothing runs


# ------------------------------------------------------------------ reference against the oracle
def _small_module():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3), torch.nn.BatchNorm2d(5), torch.nn.ReLU(),
                               torch.nn.Conv2d(5, 2, 1))


@pytest.mark.parametrize("decay", [0.5, 0.9, 0.999])
def test_reference_and_bound_against_averaged_model(decay):
    """Five perturbed updates of torch.optim.swa_utils.AveragedModel (EMA multi_avg_fn, buffers
    averaged too), each from the oracle's previous shadow: every float entry within ema_bound of the
    float64 reference, the first update an exact copy."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    m = _small_module()
    avg = AveragedModel(m, multi_avg_fn=get_ema_multi_avg_fn(decay), use_buffers=True)
    gen = torch.Generator().manual_seed(11)
    worst = 0.0
    for n in range(5):
        with torch.no_grad():
            for t in list(m.parameters()) + [b for b in m.buffers() if b.is_floating_point()]:
                t.add_(torch.randn(t.shape, generator=gen) * (0.1 + t.abs()))
        prev = {k: v.clone() for k, v in avg.module.state_dict().items()}
        avg.update_parameters(m)
        w = ref.weight32(n, decay)
        cur, new = m.state_dict(), avg.module.state_dict()
        assert list(new) == list(cur)
        for k, v in new.items():
            if not v.is_floating_point():
                continue
            if n == 0:
                assert torch.equal(v, cur[k]), k
                continue
            err = (v.double() - ref.ema_step(prev[k], cur[k], w)).abs()
            ratio = float((err / ref.ema_bound(prev[k], cur[k], w)).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (k, n, ratio)
    print(f"decay {decay}: largest err/bound {worst:.3f}")


@pytest.mark.parametrize("decay", [0.5, 0.75, 0.9, 0.999, 0.9999])
def test_foreach_lerp_stays_inside_the_bound(decay):
    gen = torch.Generator().manual_seed(5)
    e, p = ref.log_gaussians(1 << 20, gen), ref.log_gaussians(1 << 20, gen)
    w = np.float32(1.0 - decay)
    got = e.clone()
    torch._foreach_lerp_([got], [p], 1.0 - decay)
    ratio = float(((got.double() - ref.ema_step(e, p, w)).abs() / ref.ema_bound(e, p, w)).max())
    print(f"decay {decay}: largest err/bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("decay", [0.5, 0.75, 0.875])
def test_foreach_lerp_is_exact_on_eighths(decay):
    gen = torch.Generator().manual_seed(6)
    e, p = ref.eighths(1 << 16, gen), ref.eighths(1 << 16, gen)
    got = e.clone()
    torch._foreach_lerp_([got], [p], 1.0 - decay)
    assert torch.equal(got.double(), ref.ema_step(e, p, np.float32(1.0 - decay)))


def test_decay_schedule():
    from stfunet import ema
    want = [(1 + n) / (10 + n) for n in range(10)]
    assert want[0] == 0.1 and want[9] == 10 / 19
    for fn in (ref.decay_at, ema.decay_at):
        assert [fn(n, 0.999, True) for n in range(10)] == want
        assert [fn(n, 0.999, False) for n in range(10)] == [0.999] * 10
        assert [fn(n, 0.3, True) for n in range(4)] == [0.1, 2 / 11, 0.25, 0.3]      # 4/13 > 0.3
        # (1 + n) / (10 + n) reaches 0.999 at n = 8990 (8991 / 9000)
        assert fn(8989, 0.999, True) == 8990 / 8999 < 0.999
        assert fn(8990, 0.999, True) == 0.999 and fn(10 ** 6, 0.999, True) == 0.999
    for n, d, wu in [(0, 0.999, False), (1, 0.999, False), (1, 0.999, True), (7, 0.9, True), (9000, 0.999, True)]:
        w = ema.ema_weight(n, d, wu)
        assert w == float(ref.weight32(n, d, wu)) and np.float32(w) == w
    assert ema.ema_weight(0, 0.5) == 1.0 and ema.ema_weight(3, 1.0) == 0.0 and ema.ema_weight(3, 0.0) == 1.0


# ------------------------------------------------------------------ segment builder
def _check_layout(lay):
    covered = 0
    for (_, off, n), nxt in zip(lay.segs, lay.segs[1:] + [(None, lay.total, 0)]):
        assert off % 4 == 0 and n >= 0
        assert off + n <= nxt[1]                    # in order, no overlap
        covered = off + ((n + 3) & ~3)
    assert lay.total % 4 == 0 and covered == lay.total


def test_segments_of_scattered_parameters():
    from stfunet.ema import ema_segments
    lay = ema_segments([1000, 2000, 3004, 4000], [5, 8, 3, 1], [5000, 6000], [6, 6])
    assert lay.segs == [(1000, 0, 5), (2000, 8, 8), (3004, 16, 3), (4000, 20, 1), (5000, 24, 6), (6000, 32, 6)]
    assert lay.param_offsets == [0, 8, 16, 20] and lay.buffer_offsets == [24, 32] and lay.total == 40
    _check_layout(lay)
    lay = ema_segments([1000], [7])
    assert lay.segs == [(1000, 0, 7)] and lay.total == 8 and lay.buffer_offsets == []
    lay = ema_segments([], [], [64], [3])
    assert lay.segs == [(64, 0, 3)] and lay.total == 4


def test_segments_of_a_unet_layout():
    """UNet(8, 2, 8): ONE segment over the flat parameter buffer (padding included) and one per
    running_mean / running_var, every offset a multiple of 4, no overlap, total = shadow size."""
    from stfunet import UNet
    from stfunet.ema import ema_segments
    from stfunet.flat import FlatParams
    m = UNet(8, 2, 8)
    flat = FlatParams(m)
    base = 1 << 30
    nums = [p.numel() for p in flat.params]
    assert any(n % 4 for n in nums)
    bufs = [b for b in m.buffers() if b.is_floating_point()]
    bptrs = [(2 << 30) + 512 * i for i in range(len(bufs))]
    lay = ema_segments([base + 4 * o for o in flat.offsets], nums, bptrs, [b.numel() for b in bufs], flat.offsets)
    assert lay.segs[0] == (base, 0, flat.numel) and lay.param_offsets == flat.offsets
    assert len(lay.segs) == 1 + len(bufs) and len(bufs) == 2 * sum(
        isinstance(x, torch.nn.BatchNorm2d) for x in m.modules())
    assert [s[0] for s in lay.segs[1:]] == bptrs and [s[2] for s in lay.segs[1:]] == [b.numel() for b in bufs]
    assert lay.buffer_offsets[0] == flat.numel
    _check_layout(lay)
    assert lay.total == flat.numel + sum((b.numel() + 3) & ~3 for b in bufs)
    # parameters that are not where the flat layout says are refused
    with pytest.raises(ValueError, match="flat"):
        ema_segments([base + 4 * o + (4 if i == 3 else 0) for i, o in enumerate(flat.offsets)], nums, [], [],
                     flat.offsets)


# ------------------------------------------------------------------ argument checks
def _table(*segs):
    from stfunet import _lib
    return (_lib.EmaSeg * len(segs))(*[_lib.EmaSeg(p, o, n) for p, o, n in segs])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_entry_points_reject_bad_arguments_without_launch(dtype):
    from stfunet import _lib
    lib = _lib.load(dtype)
    ok = _table((FAKE, 0, 5), (FAKE + 4096, 8, 3))

    def update(shadow=FAKE, segs=FAKE, host=ok, count=2, w=0.5):
        return lib.stf_ema_update(shadow, segs, host, count, w, None)

    def swap(shadow=FAKE, segs=FAKE, host=ok, count=2):
        return lib.stf_ema_swap(shadow, segs, host, count, None)

    for fn in (update, swap):
        assert fn(shadow=None) == EINVAL
        assert fn(segs=None) == EINVAL
        assert fn(host=None) == EINVAL
        assert fn(count=0) == EINVAL and fn(count=-1) == EINVAL
        assert fn(shadow=FAKE + 4) == EINVAL and fn(shadow=FAKE + 8) == EINVAL       # not 16-byte aligned
        assert fn(host=_table((FAKE, 0, 5), (FAKE, -4, 3))) == EINVAL               # a negative offset
        assert fn(host=_table((FAKE, 0, 5), (FAKE, 8, -1))) == EINVAL               # a negative length
        assert fn(host=_table((FAKE, 0, 5), (FAKE, 6, 3))) == EINVAL                # off % 4 != 0
        assert fn(host=_table((FAKE, 2, 1)), count=1) == EINVAL
        assert fn(host=_table((FAKE, 0, 5), (None, 8, 3))) == EINVAL                # null model, len > 0
        # every segment empty (a null model is allowed there): accepted, nothing to launch
        assert fn(host=_table((None, 0, 0), (FAKE, 4, 0))) == 0
    for bad in (float("nan"), -0.1, 1.5, float("inf"), -float("inf")):
        assert update(w=bad) == EINVAL
    # w == 0 leaves the shadow as it is: accepted without a launch
    assert update(w=0.0) == 0


# ------------------------------------------------------------------ public surface
def test_weight_ema_refuses_the_host_and_bad_decays():
    import stfunet
    from stfunet.ema import WeightEMA
    assert stfunet.WeightEMA is WeightEMA and "WeightEMA" in stfunet.__all__
    m = stfunet.UNet(8, 2, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        WeightEMA(m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        WeightEMA(_small_module(), decay=0.9, warmup=True, buffers=False)
    for bad in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match="decay"):
            WeightEMA(m, decay=bad)
    sig = inspect.signature(WeightEMA.__init__)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[2:]] == [("decay", 0.999), ("warmup", False),
                                                                              ("buffers", True)]


def test_engine_options_are_keyword_only_and_default_to_none():
    from stfunet import engine
    for fn in (engine.train_one_epoch, engine.evaluate, engine.checkpoint_dict, engine.resume_from):
        par = inspect.signature(fn).parameters["ema"]
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None, fn.__name__
    assert list(inspect.signature(engine.evaluate).parameters)[:4] == ["model", "data_loader", "device",
                                                                       "num_classes"]


class _FakeEma:
    def __init__(self):
        self.loaded = None

    def state_dict(self):
        return {"decay": 0.9, "warmup": False, "num_updates": 3, "shadow": {}}

    def load_state_dict(self, sd):
        self.loaded = sd


def test_checkpoint_dict_and_resume_carry_the_average_only_when_given():
    import stfunet
    from stfunet import engine
    m = stfunet.UNet(8, 2, 8)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    sch = engine.create_lr_scheduler(opt, 4, 3)
    assert set(engine.checkpoint_dict(m, opt, sch, 5, {}, ema=None)) == {"model", "optimizer", "lr_scheduler",
                                                                         "epoch", "args"}
    fake = _FakeEma()
    ck = engine.checkpoint_dict(m, opt, sch, 5, {}, ema=fake)
    assert set(ck) == {"model", "optimizer", "lr_scheduler", "epoch", "args", "ema"} and ck["ema"]["num_updates"] == 3
    assert engine.resume_from(ck, m, opt, sch, ema=fake) == 6 and fake.loaded is ck["ema"]
    other = _FakeEma()
    del ck["ema"]                                   # a checkpoint from before the option existed
    assert engine.resume_from(ck, m, opt, sch, ema=other) == 6 and other.loaded is None
