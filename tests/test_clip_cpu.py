"""Gradient clipping, the parts that need no GPU: the segment builder, the entry points'
argument checks (nothing is launched), the partial-row query, the optimizer option's state-dict
round trip and the public signatures."""
import ctypes
import inspect

import pytest
import torch

EINVAL = 100001
FAKE = ctypes.c_void_p(1 << 20)         # a non-null, 16-byte aligned "device" address: nothing runs


# ------------------------------------------------------------------ segment builder
def test_segments_merge_only_across_multiples_of_four():
    from stfunet.flat import grad_segments
    # numels 8, 6, 4, 4, 3 at the FlatParams offsets 0, 8, 16, 20, 24
    offs, nums = [0, 8, 16, 20, 24], [8, 6, 4, 4, 3]
    assert grad_segments(offs, nums, [True] * 5) == [(0, 14), (16, 11)]
    # nothing is a multiple of 4: one segment per parameter, none spans padding
    assert grad_segments([0, 4, 8], [3, 1, 2], [True] * 3) == [(0, 3), (4, 1), (8, 2)]
    # all multiples of 4: one run
    assert grad_segments([0, 4, 12], [4, 8, 64], [True] * 3) == [(0, 76)]
    # a multiple of 4 that does not touch its neighbour (a foreign layout) is not merged
    assert grad_segments([0, 8], [4, 4], [True, True]) == [(0, 4), (8, 4)]


def test_segments_unselected_parameters_split_runs():
    from stfunet.flat import grad_segments
    offs, nums = [0, 4, 8, 12, 16], [4, 4, 4, 4, 4]
    assert grad_segments(offs, nums, [True, True, False, True, True]) == [(0, 8), (12, 8)]
    assert grad_segments(offs, nums, [False, True, True, True, False]) == [(4, 12)]
    assert grad_segments(offs, nums, [False, False, False, False, True]) == [(16, 4)]
    assert grad_segments(offs, nums, [False] * 5) == []
    assert grad_segments([], [], []) == []


def test_segments_of_a_model_cover_exactly_the_trainable_parameters():
    from stfunet import UNet
    from stfunet.flat import FlatParams, grad_segments
    m = UNet(in_channels=8, num_classes=2, base_c=8)
    m.enc1.requires_grad_(False)
    flat = FlatParams(m)
    nums = [p.numel() for p in flat.params]
    segs = grad_segments(flat.offsets, nums, flat.requires_grad_flags())
    covered = set()
    for off, n in segs:
        assert off % 4 == 0 and n > 0
        covered.update(range(off, off + n))
    want = set()
    for p, off in zip(flat.params, flat.offsets):
        if p.requires_grad:
            want.update(range(off, off + p.numel()))
    assert covered == want and sum(n for _, n in segs) == len(want)


# ------------------------------------------------------------------ argument checks
def _table(*segs):
    from stfunet import _lib
    return (_lib.Seg * len(segs))(*[_lib.Seg(o, n) for o, n in segs])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_entry_points_reject_bad_arguments_without_launch(dtype):
    from stfunet import _lib
    lib = _lib.load(dtype)
    ok = _table((0, 5), (8, 3))
    nan = float("nan")

    def norm(buf=FAKE, segs=FAKE, host=ok, count=2, max_norm=1.0, partial=FAKE, out=FAKE):
        return lib.stf_grad_norm(buf, segs, host, count, None, max_norm, partial, out, None)

    def scale(buf=FAKE, segs=FAKE, host=ok, count=2, clip=FAKE):
        return lib.stf_grad_scale(buf, segs, host, count, clip, None)

    for fn in (norm, scale):
        assert fn(buf=None) == EINVAL
        assert fn(segs=None) == EINVAL
        assert fn(host=None) == EINVAL
        assert fn(count=0) == EINVAL and fn(count=-1) == EINVAL
        assert fn(host=_table((0, 5), (8, -1))) == EINVAL            # a negative length
        assert fn(host=_table((0, 5), (6, 3))) == EINVAL             # an offset not a multiple of 4
        assert fn(host=_table((2, 1)), count=1) == EINVAL
    assert norm(partial=None) == EINVAL and norm(out=None) == EINVAL
    for bad in (nan, 0.0, -1.0):
        assert norm(max_norm=bad) == EINVAL
    assert scale(clip=None) == EINVAL

    def adamw(p=FAKE, g=FAKE, m=FAKE, v=FAKE, n=16, hyper=FAKE, clip=FAKE):
        return lib.stf_adamw_clip(p, g, m, v, n, hyper, None, None, clip, 0.9, 0.999, 1e-8, 1e-2, None)

    assert adamw(hyper=None) == EINVAL and adamw(clip=None) == EINVAL and adamw(n=-1) == EINVAL
    for name in ("p", "g", "m", "v"):
        assert adamw(**{name: None}) == EINVAL


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_grad_norm_rows_positive_monotone_bounded(dtype):
    from stfunet import _lib
    lib = _lib.load(dtype)
    ns = [0, 1, 3, 4, 4095, 4096, 4097, 1 << 20, (1 << 20) + 7, 31_046_466, 1 << 31, 1 << 40, (1 << 62)]
    rows = [lib.stf_grad_norm_rows(n) for n in ns]
    assert all(r >= 1 for r in rows)
    assert rows == sorted(rows)
    assert max(rows) <= 2048                     # the bound the header states
    assert rows[0] == 1 and rows[5] == 1 and rows[6] == 2
    assert lib.stf_grad_norm_rows(-5) == 1


# ------------------------------------------------------------------ optimizer option, signatures
def test_adamw_max_grad_norm_state_dict_round_trip():
    from stfunet.optim import AdamW
    ps = [torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(3, 4))]
    opt = AdamW(ps, lr=1e-3, max_grad_norm=0.5)
    assert opt.param_groups[0]["max_grad_norm"] == 0.5 and opt.grad_norm is None
    sd = opt.state_dict()
    assert sd["param_groups"][0]["max_grad_norm"] == 0.5
    other = AdamW(ps, lr=1e-3)
    assert other.param_groups[0]["max_grad_norm"] is None
    other.load_state_dict(sd)
    assert other.param_groups[0]["max_grad_norm"] == 0.5
    # a checkpoint written before the option existed
    old = AdamW(ps, lr=1e-3).state_dict()
    for group in old["param_groups"]:
        del group["max_grad_norm"]
    opt.load_state_dict(old)
    assert opt.param_groups[0]["max_grad_norm"] is None
    # set later, as any torch hyper-parameter
    opt.param_groups[0]["max_grad_norm"] = 2.0
    assert opt.state_dict()["param_groups"][0]["max_grad_norm"] == 2.0


def test_clip_grad_norm_refuses_other_norm_types():
    import stfunet
    from stfunet.optim import clip_grad_norm_
    assert stfunet.clip_grad_norm_ is clip_grad_norm_
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(ValueError, match="L2"):
        clip_grad_norm_([p], 1.0, norm_type=1)
    with pytest.raises(ValueError, match="L2"):
        clip_grad_norm_([p], 1.0, norm_type=float("inf"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        clip_grad_norm_([p], 1.0)
    assert torch.equal(p.grad, torch.ones(4))
    q = torch.nn.Parameter(torch.zeros(4))                 # no gradient anywhere: the norm of nothing
    assert float(clip_grad_norm_([q], 1.0)) == 0.0


def test_train_one_epoch_has_the_keyword_only_option():
    from stfunet import engine
    sig = inspect.signature(engine.train_one_epoch)
    par = sig.parameters["max_grad_norm"]
    assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None
    # the reference's positional surface is as it was
    assert list(sig.parameters)[:9] == ["model", "optimizer", "data_loader", "device", "epoch", "num_classes",
                                        "lr_scheduler", "print_freq", "scaler"]
