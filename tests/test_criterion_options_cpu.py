"""Criterion options on the CPU: the tests' restatement against the reference-generated
fixture, and the argument checks of ``stfunet.criterion`` and of the C entry points
(no kernel launches)."""
import ctypes

import pytest
import torch

from _criterion_ref import fixture_entries, ref_loss_and_grad

ENTRIES = fixture_entries()
EINVAL = 100001


def test_fixture_covers_the_option_grid():
    got = {(e["logits"].shape[1], e["weight"] is not None, e["dice"], e["ignore_index"]) for e in ENTRIES}
    want = {(k, w, d, i) for k in (2, 3) for w in (False, True) for d in (False, True) for i in (-100, 255)}
    assert got == want and len(ENTRIES) == 16
    for e in ENTRIES:
        assert e["logits"].shape == (3, e["logits"].shape[1], 8, 12)
        if e["ignore_index"] == 255:
            t = e["target"]
            assert (t[0, :, 9:] == 255).all() and (t[0, :, :9] != 255).all()
            assert (t[1, 6:] == 255).all() and (t[1, :6] != 255).all() and (t[2] == 255).all()


@pytest.mark.parametrize("e", ENTRIES, ids=[e["name"] for e in ENTRIES])
def test_restatement_equals_reference(e):
    loss, grad = ref_loss_and_grad(e["logits"], e["target"], e["weight"], e["ignore_index"], e["dice"])
    print(e["name"], "loss", loss, "ref", e["loss"], "max |dgrad|", (grad - e["grad"].double()).abs().max().item())
    assert abs(loss - e["loss"]) < 1e-6
    assert (grad - e["grad"].double()).abs().max().item() < 1e-6
    if e["ignore_index"] >= 0:
        assert (e["grad"].permute(0, 2, 3, 1)[e["target"] == e["ignore_index"]] == 0).all()


def test_restatement_all_ignored_batch_is_nan():
    loss, _ = ref_loss_and_grad(torch.randn(2, 2, 4, 4), torch.full((2, 4, 4), 255), None, 255, True)
    assert loss != loss


def test_criterion_rejects_bad_options():
    from stfunet import criterion
    from stfunet.loss import ce_dice_loss
    x, t = torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="ignore_index"):
        criterion({"out": x}, t, ignore_index=1, num_classes=2)
    with pytest.raises(ValueError, match="loss_weight"):
        criterion({"out": x}, t, loss_weight=[1.0, 2.0, 3.0], num_classes=2)
    with pytest.raises(ValueError, match="loss_weight"):
        criterion({"out": x}, t, loss_weight=torch.ones(3), num_classes=2)
    with pytest.raises(ValueError, match="ignore_index"):
        ce_dice_loss(x, t, ignore_index=0)
    # valid options on a CPU tensor reach the device guard: no eager fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        criterion({"out": x}, t, loss_weight=[1.0, 2.0], ignore_index=255, dice=False)


def test_train_one_epoch_keeps_the_reference_positional_signature():
    import inspect
    from stfunet import engine
    ps = inspect.signature(engine.train_one_epoch).parameters
    names = list(ps)
    assert names[:9] == ["model", "optimizer", "data_loader", "device", "epoch", "num_classes", "lr_scheduler",
                         "print_freq", "scaler"]
    for n, d in (("loss_weight", None), ("dice", True), ("ignore_index", -100)):
        assert ps[n].kind is inspect.Parameter.KEYWORD_ONLY and ps[n].default == d


def test_library_rejects_bad_loss_options_without_launch():
    from stfunet import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(1 << 20)          # fake non-null pointers: nothing runs
    fwd = lambda K, ign, w=None: lib.stf_loss_opt_fwd(fake, fake, 1, 4, 4, K, w, ign, 1, fake, fake, None)  # noqa
    bwd = lambda K, ign, w=None: lib.stf_loss_opt_bwd(fake, fake, 1, 4, 4, K, w, ign, 1, fake, fake, fake,  # noqa
                                                      None)
    for f in (fwd, bwd):
        assert f(2, 1) == EINVAL             # ignore_index is a class id
        assert f(2, 0) == EINVAL
        assert f(3, 2, fake) == EINVAL
        assert f(0, 255) == EINVAL           # classes outside 1..4
        assert f(5, 255, fake) == EINVAL
    assert lib.stf_loss_opt_scratch_floats(3, 2) == 3 * 2 * 3 + 2 + 3 * 64 * (3 * 2 + 2)
    assert lib.stf_abi_version() == 17
