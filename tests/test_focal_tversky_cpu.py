"""Focal cross-entropy and Tversky overlap on the CPU: the tests' restatement pinned to the criterion's
own restatement at gamma = 0, alpha = beta = 1/2 and to the closed-form gradient the kernels implement;
the three new entry points' surface, argument checks and scratch size (no kernel launches); the
``ValueError`` cases, the signatures and the routing of ``stfunet.criterion``."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import _criterion_ref
import _focal_ref
from _criterion_ref import fixture_entries
from conftest import REPO

EINVAL = 100001
NEW = ["stf_loss_ft_scratch_floats", "stf_loss_ft_fwd", "stf_loss_ft_bwd"]
NAN, INF = float("nan"), float("inf")


def _k7_case():
    g = torch.Generator().manual_seed(7)
    logits = torch.randn(3, 7, 7, 9, generator=g) * 3.0
    target = torch.randint(0, 7, (3, 7, 9), generator=g)
    target[0, :, 6:] = 255
    target[1, 5:] = 255
    target[2] = 255
    return dict(name="k7_weight_ignore", logits=logits, target=target,
                weight=torch.tensor([0.5 + 0.75 * k for k in range(7)]), ignore_index=255, dice=True)


CASES = fixture_entries() + [_k7_case()]
IDS = [e["name"] for e in CASES]


@pytest.mark.parametrize("e", CASES, ids=IDS)
def test_restatement_is_the_criterion_at_neutral_values(e):
    loss, grad = _focal_ref.ref_loss_and_grad(e["logits"], e["target"], e["weight"], e["ignore_index"], e["dice"],
                                              gamma=0.0, alpha=0.5, beta=0.5)
    want, wgrad = _criterion_ref.ref_loss_and_grad(e["logits"], e["target"], e["weight"], e["ignore_index"], e["dice"])
    dg = (grad - wgrad).abs().max().item()
    print(e["name"], "|dloss|", abs(loss - want), "max |dgrad|", dg)
    assert abs(loss - want) < 1e-12 and dg < 1e-12


@pytest.mark.parametrize("alpha,beta", [(0.3, 0.7), (0.7, 0.3)])
@pytest.mark.parametrize("gamma", [0.5, 2.0])
@pytest.mark.parametrize("e", CASES, ids=IDS)
def test_closed_form_gradient_is_autograd_of_the_restatement(e, gamma, alpha, beta):
    args = (e["logits"].double(), e["target"], None if e["weight"] is None else e["weight"].double(),
            e["ignore_index"], e["dice"], gamma, alpha, beta)
    _, grad = _focal_ref.ref_loss_and_grad(*args)
    closed = _focal_ref.closed_form_grad(*args)
    d = (closed - grad).abs().max().item()
    print(e["name"], gamma, alpha, beta, "max |closed - autograd|", d, "max |grad|", grad.abs().max().item())
    assert d < 1e-10
    assert grad.abs().max().item() > 1e-6


def test_restatement_edges():
    """gamma and the Tversky pair move the loss; K = 1 (1-q exactly 0) is finite with a zero gradient;
    saturated logits are finite; an all-ignored batch is NaN."""
    e = _k7_case()
    base, _ = _focal_ref.ref_loss_and_grad(e["logits"], e["target"], e["weight"], 255, True)
    foc, _ = _focal_ref.ref_loss_and_grad(e["logits"], e["target"], e["weight"], 255, True, gamma=2.0)
    tv, _ = _focal_ref.ref_loss_and_grad(e["logits"], e["target"], e["weight"], 255, True, alpha=0.3, beta=0.7)
    assert foc < base - 1e-3 and abs(tv - base) > 1e-4
    loss1, grad1 = _focal_ref.ref_loss_and_grad(torch.randn(2, 1, 4, 4), torch.zeros(2, 4, 4, dtype=torch.long),
                                                gamma=0.5, alpha=0.3, beta=0.7)
    assert loss1 == loss1 and grad1.abs().max().item() < 1e-12
    sat = torch.tensor([60.0, -60.0]).reshape(1, 2, 1, 1).expand(1, 2, 4, 4).contiguous()
    tgt = torch.zeros(1, 4, 4, dtype=torch.long)
    tgt[0, 2:] = 1
    for gamma in (0.5, 2.0):
        loss, grad = _focal_ref.ref_loss_and_grad(sat, tgt, gamma=gamma)
        assert torch.isfinite(grad).all() and loss == loss and abs(loss) < 1e6
        assert torch.allclose(grad, _focal_ref.closed_form_grad(sat.double(), tgt, gamma=gamma), rtol=0, atol=1e-10)
    nan, _ = _focal_ref.ref_loss_and_grad(torch.randn(2, 2, 4, 4), torch.full((2, 4, 4), 255), None, 255, True, 2.0)
    assert nan != nan


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_new_symbols_declared_exported_and_typed(dtype):
    from stfunet import _lib
    header = open(os.path.join(REPO, "include", "stfunet.h")).read()
    lib = _lib.load(dtype)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _lib.EXPORTED and hasattr(lib, s), s
    f, P, i = ctypes.c_float, ctypes.c_void_p, ctypes.c_int
    assert _lib._SIGS["stf_loss_ft_scratch_floats"] == (i, [i, i])
    assert _lib._SIGS["stf_loss_ft_fwd"] == (i, [P, P, i, i, i, i, P, i, i, f, f, f, P, P, P])
    assert _lib._SIGS["stf_loss_ft_bwd"] == (i, [P, P, i, i, i, i, P, i, i, f, f, f, P, P, P, P])
    # the many-class argument lists with three floats after ``dice``
    for name in ("fwd", "bwd"):
        mc, ft = _lib._SIGS[f"stf_loss_mc_{name}"][1], _lib._SIGS[f"stf_loss_ft_{name}"][1]
        assert ft[:9] == mc[:9] and ft[9:12] == [f, f, f] and ft[12:] == mc[9:]
    # the header declares them in that order
    for name in ("stf_loss_ft_fwd", "stf_loss_ft_bwd"):
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, header).group(1)
        assert re.search(r"int dice,\s*float focal_gamma,\s*float tversky_alpha,\s*float tversky_beta,", decl), decl


def test_library_rejects_bad_focal_tversky_arguments_without_launch():
    from stfunet import _lib
    for dtype in (torch.bfloat16, torch.float16):
        lib = _lib.load(dtype)
        fake = ctypes.c_void_p(1 << 20)          # fake non-null pointers: nothing runs

        def fwd(K=2, ign=255, g=2.0, a=0.3, b=0.7, N=1, w=None, lg=fake, tg=fake, tm=fake, out=fake):
            return lib.stf_loss_ft_fwd(lg, tg, N, 4, 4, K, w, ign, 1, g, a, b, tm, out, None)

        def bwd(K=2, ign=255, g=2.0, a=0.3, b=0.7, N=1, w=None, lg=fake, tg=fake, tm=fake, out=fake):
            return lib.stf_loss_ft_bwd(lg, tg, N, 4, 4, K, w, ign, 1, g, a, b, tm, fake, out, None)

        for f in (fwd, bwd):
            assert f(K=0) == EINVAL and f(K=17, w=fake) == EINVAL and f(K=-3, ign=-100) == EINVAL
            assert f(K=2, ign=1) == EINVAL and f(K=7, ign=0, w=fake) == EINVAL and f(K=16, ign=15) == EINVAL
            assert f(N=0) == EINVAL and f(N=65536) == EINVAL
            assert f(g=-0.5) == EINVAL and f(g=NAN) == EINVAL and f(g=INF) == EINVAL
            assert f(a=-0.1) == EINVAL and f(b=-0.1) == EINVAL and f(a=NAN) == EINVAL and f(b=INF) == EINVAL
            assert f(a=0.0, b=0.0) == EINVAL
            for null in ("lg", "tg", "tm", "out"):
                assert f(**{null: None}) == EINVAL, null
        assert lib.stf_loss_ft_fwd(fake, fake, 1, 0, 4, 2, None, 255, 1, 2.0, 0.3, 0.7, fake, fake, None) == EINVAL
        assert lib.stf_loss_ft_bwd(fake, fake, 1, 4, 0, 2, None, 255, 1, 2.0, 0.3, 0.7, fake, fake, fake, None) == EINVAL


def test_scratch_floats_is_the_many_class_formula():
    from stfunet import _lib
    lib = _lib.load()
    for N, K in ((1, 1), (2, 2), (3, 5), (65, 16), (2, 9), (64, 4)):
        assert lib.stf_loss_ft_scratch_floats(N, K) == N * K * 3 + 2 + N * 64 * (3 * K + 2)
        assert lib.stf_loss_ft_scratch_floats(N, K) == lib.stf_loss_mc_scratch_floats(N, K)
    assert lib.stf_loss_ft_scratch_floats(3, 0) == 0 and lib.stf_loss_ft_scratch_floats(3, 17) == 0


BAD = [dict(focal_gamma=-1.0), dict(focal_gamma=NAN), dict(focal_gamma=INF), dict(tversky=0.5),
       dict(tversky=(0.5,)), dict(tversky=(0.3, 0.3, 0.4)), dict(tversky=(-0.1, 0.5)), dict(tversky=(0.5, NAN)),
       dict(tversky=(INF, 0.5)), dict(tversky=(0.0, 0.0)), dict(tversky=("a", "b")),
       dict(tversky=(0.3, 0.7), dice=False)]


@pytest.mark.parametrize("kw", BAD, ids=[repr(kw) for kw in BAD])
def test_criterion_rejects_bad_focal_tversky_values(kw):
    from stfunet import criterion
    from stfunet.loss import ce_dice_loss
    x, t = torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="focal_gamma|tversky"):
        criterion({"out": x}, t, **kw)
    with pytest.raises(ValueError, match="focal_gamma|tversky"):
        ce_dice_loss(x, t, **kw)


def test_valid_values_reach_the_device_guard():
    from stfunet import criterion
    x, t = torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long)
    for kw in (dict(focal_gamma=2.0), dict(tversky=(0.3, 0.7)), dict(tversky=[0.0, 1.0], focal_gamma=0.5),
               dict(focal_gamma=1.0, dice=False)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):          # no eager fallback
            criterion({"out": x}, t, **kw)


def test_signatures():
    from stfunet import criterion, engine
    from stfunet.loss import ce_dice_loss
    ps = inspect.signature(criterion).parameters
    assert list(ps) == ["inputs", "target", "loss_weight", "num_classes", "dice", "ignore_index", "focal_gamma",
                        "tversky"]
    assert [ps[n].default for n in list(ps)[2:]] == [None, 2, True, -100, 0.0, None]
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in ps.values())
    ps = inspect.signature(ce_dice_loss).parameters
    assert list(ps) == ["logits", "target", "weight", "ignore_index", "dice", "focal_gamma", "tversky"]
    assert [ps[n].default for n in list(ps)[2:]] == [None, -100, True, 0.0, None]
    ps = inspect.signature(engine.train_one_epoch).parameters
    assert list(ps)[:9] == ["model", "optimizer", "data_loader", "device", "epoch", "num_classes", "lr_scheduler",
                            "print_freq", "scaler"]
    for n, d in (("loss_weight", None), ("dice", True), ("ignore_index", -100), ("focal_gamma", 0.0),
                 ("tversky", None)):
        assert ps[n].kind is inspect.Parameter.KEYWORD_ONLY and ps[n].default == d


def _record_routes(monkeypatch):
    """``stfunet.loss.call`` replaced with a recorder that launches nothing; the autograd function then
    runs on CPU tensors."""
    from stfunet import loss
    calls = []
    monkeypatch.setattr(loss, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(loss, "stream", lambda: None)

    def route(K, weight=None, ignore_index=-100, dice=True, focal_gamma=0.0, tversky=None):
        del calls[:]
        x = torch.zeros(2, K, 4, 4, requires_grad=True)
        t = torch.zeros(2, 4, 4, dtype=torch.long)
        w = loss._class_weight(weight, K)
        out = loss._CEDice.apply(x, t, w, ignore_index, dice, loss._focal_tversky(focal_gamma, tversky, dice))
        out.backward()
        assert len(calls) == 2
        return calls[0], calls[1]
    return route


def test_default_values_take_the_three_existing_routes(monkeypatch):
    route = _record_routes(monkeypatch)
    for kw in (dict(), dict(focal_gamma=0.0, tversky=None), dict(focal_gamma=0, tversky=None)):
        (f, fa), (b, ba) = route(2, **kw)
        assert (f, b) == ("stf_loss_fwd", "stf_loss_bwd") and len(fa) == 9 and len(ba) == 10
        (f, fa), (b, ba) = route(2, weight=[1.0, 2.0], ignore_index=255, **kw)
        assert (f, b) == ("stf_loss_opt_fwd", "stf_loss_opt_bwd") and len(fa) == 12 and len(ba) == 13
        assert fa[7:9] == (255, 1)
        (f, fa), (b, ba) = route(7, **kw)
        assert (f, b) == ("stf_loss_mc_fwd", "stf_loss_mc_bwd") and len(fa) == 12 and len(ba) == 13
        assert fa[6:9] == (None, -100, 1)


@pytest.mark.parametrize("K", [2, 7])
def test_any_other_value_takes_the_focal_tversky_route(monkeypatch, K):
    route = _record_routes(monkeypatch)
    for kw, want in ((dict(focal_gamma=2.0), (2.0, 0.5, 0.5)), (dict(tversky=(0.3, 0.7)), (0.0, 0.3, 0.7)),
                     (dict(tversky=(0.5, 0.5)), (0.0, 0.5, 0.5)), (dict(focal_gamma=1e-3, dice=False), (1e-3, 0.5, 0.5)),
                     (dict(focal_gamma=0.5, tversky=[0.7, 0.3], weight=[1.0] * K, ignore_index=255), (0.5, 0.7, 0.3))):
        (f, fa), (b, ba) = route(K, **kw)
        assert (f, b) == ("stf_loss_ft_fwd", "stf_loss_ft_bwd"), kw
        assert len(fa) == 15 and len(ba) == 16
        assert fa[2:6] == (2, 4, 4, K) and fa[7] == kw.get("ignore_index", -100) and fa[8] == int(kw.get("dice", True))
        assert fa[9:12] == want and ba[9:12] == want
        assert (fa[6] is None) == ("weight" not in kw)


def test_criterion_passes_the_values_to_every_head(monkeypatch):
    from stfunet import loss
    seen = []

    def fake(x, target, weight, ignore_index, dice, focal_gamma, tversky):
        seen.append((focal_gamma, tversky))
        return x.sum()

    monkeypatch.setattr(loss, "ce_dice_loss", fake)
    x, t = torch.ones(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long)
    both = loss.criterion({"out": x, "aux": 2 * x}, t, focal_gamma=2.0, tversky=(0.3, 0.7))
    assert seen == [(2.0, (0.3, 0.7))] * 2 and both.item() == 32 + 0.5 * 64
