"""Frozen-parameter training on the GPU: ``requires_grad_(False)`` and ``.eval()`` on a submodule mean
what they mean in torch, and the step skips the backward nothing trainable needs.

Everything that compares the frozen step with the all-trainable one is bitwise (``torch.equal``): the
frozen step launches a subset of the same kernels on the same operands.  Shapes: ``STFLSTMUNet(T=3)``,
B=2, 40x48 frames (not divisible by 32: the decoder's bilinear size fallback; layer1 has 120 pixels
per step = two LSTM workgroups, the second ragged), the same with PK maps, ``UNet(3, base_c=8)`` at
B=2, 32x32; bf16 storage, plus one fp16 case per model.
"""
import contextlib
import copy
import os

import pytest
import torch

import _launch_trace as lt

pytestmark = pytest.mark.gpu
DEV = "cuda"
T, B, H, W = 3, 2, 40, 48
STF_ENC = ("conv1", "bn1", "layer1", "layer2", "layer3", "layer4")
STF_DEC = ("decoder4", "decoder3", "decoder2", "upconv1", "final_res", "final")
UNET_ENC = ("enc1", "enc2", "enc3", "enc4")
UNET_DEC = ("up4", "dec4", "up3", "dec3", "up2", "dec2", "up1", "dec1", "out_conv")


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


def _model(which, dtype=torch.bfloat16):
    from stfunet import STFLSTMUNet, UNet
    torch.manual_seed(0)
    if which == "unet":
        m = UNet(in_channels=3, num_classes=2, base_c=8)
    else:
        m = STFLSTMUNet(in_channels=1, num_classes=2, time_steps=T, use_pk_maps=which == "stf_pk")
    m.storage_dtype = dtype
    return m.to(DEV).train()


def _input(which, seed=11, hw=None):
    from stfunet.synthetic import dce_batch
    if which == "unet":
        return dce_batch(B, 3, 32, 32, seed=seed, device=DEV)[0].flatten(1, 2)
    h, w = hw or (H, W)
    return dce_batch(B, T, h, w, seed=seed, device=DEV, pk_channels=3 if which == "stf_pk" else 0)[0]


def _freeze(m, pattern):
    """``pattern``: submodule names to freeze, or ("only", name): everything but that submodule."""
    if pattern and pattern[0] == "only":
        m.requires_grad_(False)
        m.get_submodule(pattern[1]).requires_grad_(True)
    else:
        for n in pattern:
            m.get_submodule(n).requires_grad_(False)
    return m


def _step(m, x, want_dx=False, seed=5):
    """One eager-or-planned step with a fixed random dlogits; returns (logits, dx)."""
    x = x.clone().requires_grad_(want_dx)
    out = m(x)["out"]
    r = torch.randn(out.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    logits = out.detach().clone()
    (out * r).sum().backward()
    torch.cuda.synchronize()
    return logits, x.grad


_REF = {}


def _reference(which, dtype, want_dx):
    """Model A (everything trainable): its state, logits, gradients and dx, computed once per case
    (eagerly: the comparison is between schedules, plans are test 7's) and never modified after."""
    key = (which, dtype, want_dx)
    if key not in _REF:
        with _env(STF_PLAN="0"):
            a = _model(which, dtype)
            sd = copy.deepcopy(a.state_dict())
            logits, dx = _step(a, _input(which), want_dx)
        _REF[key] = dict(sd=sd, logits=logits, dx=dx,
                         grads={n: p.grad.clone() for n, p in a.named_parameters()})
    return _REF[key]


def _frozen_copy(which, dtype, pattern, ref):
    b = _model(which, dtype)
    b.load_state_dict(ref["sd"])
    return _freeze(b, pattern)


PATTERNS = [
    ("stf", STF_ENC, False), ("stf", ("only", "final"), False), ("stf", STF_DEC, False),
    ("stf", ("layer2.1",), False), ("stf_pk", STF_ENC, False), ("stf", STF_ENC, True),
    ("stf_pk", STF_ENC, True),
    ("unet", UNET_ENC, False), ("unet", ("only", "out_conv"), False), ("unet", UNET_DEC, False),
    ("unet", ("enc3",), False), ("unet", UNET_ENC, True),
]


def _check_grads(b, ref):
    n_tr = 0
    for n, p in b.named_parameters():
        if p.requires_grad:
            n_tr += 1
            assert p.grad is not None and torch.equal(p.grad, ref["grads"][n]), n
        else:
            assert p.grad is None, n
    assert n_tr > 0


@pytest.mark.parametrize("which,pattern,want_dx", PATTERNS,
                         ids=[f"{w}-{'+'.join(p)}{'-dx' if d else ''}" for w, p, d in PATTERNS])
def test_frozen_gradients_bitwise(which, pattern, want_dx):
    """B (frozen by pattern) against A (all trainable), same weights, input and dlogits: every
    trainable parameter's gradient bit for bit A's, frozen parameters without a gradient, same logits
    (and running statistics), and the input gradient equal too where it is asked for."""
    ref = _reference(which, torch.bfloat16, want_dx)
    with _env(STF_PLAN="0"):
        b = _frozen_copy(which, torch.bfloat16, pattern, ref)
        logits, dx = _step(b, _input(which), want_dx)
    assert torch.equal(logits, ref["logits"])
    _check_grads(b, ref)
    if want_dx:
        assert dx is not None and torch.equal(dx, ref["dx"])


@pytest.mark.parametrize("which,pattern", [("stf", STF_ENC), ("unet", UNET_ENC)])
def test_frozen_gradients_bitwise_fp16(which, pattern):
    ref = _reference(which, torch.float16, False)
    with _env(STF_PLAN="0"):
        b = _frozen_copy(which, torch.float16, pattern, ref)
        logits, _ = _step(b, _input(which))
    assert torch.equal(logits, ref["logits"])
    _check_grads(b, ref)


# ------------------------------------------------------------------ launch traces
def _traced_step(m, x, dtype=torch.bfloat16):
    """(forward trace, backward trace, dx arguments of the stf_lstm_seq_bwd calls) of one eager step."""
    from stfunet import _lib
    seq_dx = []
    with _env(STF_PLAN="0"), lt.tracing(dtype) as trace:
        table = _lib._FNS[dtype]
        inner = table["stf_lstm_seq_bwd"]

        def seq_bwd(*args):
            seq_dx.append(args[11])
            return inner(*args)
        table["stf_lstm_seq_bwd"] = seq_bwd
        out = m(x)["out"]
        n_fwd = len(trace)
        out.square().mean().backward()
        torch.cuda.synchronize()
    return trace[:n_fwd], trace[n_fwd:], seq_dx


def _is_subsequence(short, long):
    it = iter(long)
    return all(any(e == f for f in it) for e in short)


def _names(trace):
    return [e if isinstance(e, str) else e[0] for e in trace]


def test_launch_trace_stf_frozen_encoder():
    a, b = _model("stf"), _freeze(_model("stf"), STF_ENC)
    x = _input("stf")
    fa, ba, dxa = _traced_step(a, x)
    fb, bb, dxb = _traced_step(b, x)
    assert fb == fa                                   # the forward launches do not change
    assert _is_subsequence(bb, ba) and len(bb) < len(ba)
    names = _names(bb)
    assert "stf_stem_wgrad7" in _names(ba) and "stf_stem_wgrad7" not in names
    assert "stf_bn_bwd_reduce_pool3" in _names(ba) and "stf_bn_bwd_reduce_pool3" not in names
    assert "stf_bn_bwd_apply_pool3" not in names

    def encoder_wgrads(trace):       # the ResNet convs run on the T*B images: 3x3, or the strided 1x1 shortcut
        g = lt.GEOM
        return [e for e in trace if not isinstance(e, str) and e[0] == "stf_wgrad" and e[1 + g.index("N")] == T * B
                and (e[1 + g.index("R")] == 3 or e[1 + g.index("stride")] == 2)]
    assert len(encoder_wgrads(ba)) == 2 * 16 + 3 and not encoder_wgrads(bb)
    # lstm1 (C = 64) is the whole-sequence kernel: with dx in A, without in B
    assert len(dxa) == 1 and dxa[0] is not None
    assert len(dxb) == 1 and dxb[0] is None
    # the other LSTMs' per-step paths lose exactly their hoisted input-half GEMM
    def gemms(trace, nout, k):
        g = lt.GEOM
        return [e for e in trace if not isinstance(e, str) and e[0] == "stf_igemm" and e[-1] == nout
                and e[1 + g.index("Cs")] == k and e[1 + g.index("N")] == T * B and e[1 + g.index("R")] == 1]
    for c in (128, 256, 512):
        assert len(gemms(ba, c, 4 * c)) == 1 and not gemms(bb, c, 4 * c)


def test_launch_trace_unet_frozen_encoder(monkeypatch):
    a, b = _model("unet"), _freeze(_model("unet"), UNET_ENC)
    x = _input("unet")
    ran = []
    from stfunet.unet import DoubleConvProgram
    orig = DoubleConvProgram._backward

    def spy(self, *args, **kw):
        ran.append(self.name)
        return orig(self, *args, **kw)
    monkeypatch.setattr(DoubleConvProgram, "_backward", spy)
    fa, ba, _ = _traced_step(a, x)
    ran_a, ran[:] = list(ran), []
    fb, bb, _ = _traced_step(b, x)
    assert fb == fa
    assert _is_subsequence(bb, ba) and len(bb) < len(ba)
    assert ran_a == ["dec1", "dec2", "dec3", "dec4", "bottleneck", "enc4", "enc3", "enc2", "enc1"]
    assert ran == ["dec1", "dec2", "dec3", "dec4", "bottleneck"]        # none of the encoder levels
    # the encoder's eight weight gradients are gone, and the bottleneck's input gradient (one dgrad
    # GEMM) with the four BN backwards pairs of the levels
    assert _names(ba).count("stf_wgrad") - _names(bb).count("stf_wgrad") == 8
    assert _names(ba).count("stf_bn_bwd_reduce") - _names(bb).count("stf_bn_bwd_reduce") == 4


# ------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("P,steps", [(120, 1), (120, 3), (64, 1), (64, 3)])
def test_lstm_seq_bwd_without_dx(P, steps, dtype):
    """stf_lstm_seq_bwd with dx == NULL on random [x | h] rows: dgates bit for bit those of the launch
    with dx, and a sentinel-filled dx buffer (the one the other launch writes) untouched."""
    from stfunet import _lib
    from stfunet._lib import call, stream
    C = 64
    g = torch.Generator(device=DEV).manual_seed(1000 * P + steps)

    def rnd(*shape, scale=1.0, dt=torch.float32):
        return (torch.randn(*shape, device=DEV, generator=g) * scale).to(dt).contiguous()
    with _lib.storage(dtype):
        w_ih, w_hh = rnd(4 * C, C, scale=0.125), rnd(4 * C, C, scale=0.125)
        b_ih, b_hh = rnd(4 * C, scale=0.1), rnd(4 * C, scale=0.1)
        wcat = torch.empty(8 * C * C, dtype=dtype, device=DEV)
        wcat_t = torch.empty(8 * C * C, dtype=dtype, device=DEV)
        bias = torch.empty(4 * C, dtype=torch.float32, device=DEV)
        call("stf_lstm_pack", w_ih.data_ptr(), w_hh.data_ptr(), b_ih.data_ptr(), b_hh.data_ptr(), C,
             wcat.data_ptr(), wcat_t.data_ptr(), bias.data_ptr(), stream())
        lbuf = rnd(steps, P, 2 * C, dt=dtype)
        cst = rnd(steps, P, C)
        dh = rnd(P, C, dt=dtype)
        SENT = 0x5A5A
        outs = []
        for with_dx in (True, False):
            dg = torch.zeros(steps, P, 4 * C, dtype=dtype, device=DEV)
            dx = torch.full((steps, P, 2 * C), SENT, dtype=torch.int16, device=DEV)
            call("stf_lstm_seq_bwd", wcat.data_ptr(), wcat_t.data_ptr(), bias.data_ptr(), lbuf.data_ptr(), P, steps,
                 C, cst.data_ptr(), dh.data_ptr(), C, dg.data_ptr(), dx.data_ptr() if with_dx else None,
                 2 * C if with_dx else 0, stream())
            torch.cuda.synchronize()
            outs.append((dg, dx))
    (dg1, dx1), (dg0, dx0) = outs
    assert torch.equal(dg1.view(torch.int16), dg0.view(torch.int16))
    assert dg1.float().abs().sum() > 0 and torch.isfinite(dg1.float()).all()
    assert bool((dx0 == SENT).all())                                  # nothing written without dx
    assert bool((dx1[:, :, C:] == SENT).all()) and not bool((dx1[:, :, :C] == SENT).all())


# ------------------------------------------------------------------ training
def _batches(n, seed=700):
    from stfunet.synthetic import dce_batch
    return [dce_batch(B, T, H, W, seed=seed + i, device=DEV, mask_hw=(H // 2, W // 2)) for i in range(n)]


def _train(model, params, steps, batches, freeze_grads_of=()):
    from stfunet import engine
    from stfunet.optim import AdamW
    opt = AdamW(params, lr=1e-3, weight_decay=1e-4)
    losses = []
    for i in range(steps):
        x, t = batches[i % len(batches)]
        loss = engine.criterion(model(x), t)
        opt.zero_grad()
        for p in freeze_grads_of:              # (gradients the optimizer does not own)
            p.grad = None
        loss.backward()
        opt.step()
        losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    return torch.stack(losses), {k: v.detach().clone() for k, v in model.state_dict().items()}, opt


def _encoder_params(m):
    return [p for n in STF_ENC for p in m.get_submodule(n).parameters()]


def test_trajectory_equals_all_trainable_with_partial_optimizer():
    """8 steps of the training recipe (criterion, AdamW, plans on) with the encoder frozen, against the
    same model kept all-trainable whose optimizer owns only the non-encoder parameters -- the
    computation before freezing existed: losses, parameters and BatchNorm statistics identical."""
    batches = _batches(3)
    f = _freeze(_model("stf"), STF_ENC)
    g = _model("stf")
    g.load_state_dict(f.state_dict())
    lf, sf, _ = _train(f, [p for p in f.parameters() if p.requires_grad], 8, batches)
    enc = _encoder_params(g)
    ids = {id(p) for p in enc}
    lg, sg, _ = _train(g, [p for p in g.parameters() if id(p) not in ids], 8, batches, freeze_grads_of=enc)
    assert f.program.runtime.bwd is not None          # the frozen step was recorded and replayed
    assert torch.equal(lf, lg)
    for k in sf:
        assert torch.equal(sf[k], sg[k]), k
    moved = [k for k in sf if "running_mean" in k and k.startswith("layer")]
    assert moved and all(not torch.equal(sf[k], torch.zeros_like(sf[k])) for k in moved)


def test_plans_with_frozen_encoder_and_toggling():
    """Replayed frozen steps equal eager ones; unfreezing between steps re-records and then gives the
    gradients of a fresh all-trainable model; freezing again works too."""
    batches = _batches(2, seed=730)
    res = {}
    for plan in ("1", "0"):
        with _env(STF_PLAN=plan):
            m = _freeze(_model("stf"), STF_ENC)
            losses, state, _ = _train(m, [p for p in m.parameters() if p.requires_grad], 6, batches)
            res[plan] = (losses, state, m)
    assert res["1"][2].program.runtime.bwd is not None and res["0"][2].program.runtime.bwd is None
    assert torch.equal(res["1"][0], res["0"][0])
    for k in res["1"][1]:
        assert torch.equal(res["1"][1][k], res["0"][1][k]), k
    with _env(STF_PLAN="1"):               # (the STF_* environment is part of a plan's signature)
        m = res["1"][2]
        rt = m.program.runtime
        frozen_entry = rt.cur
        x = _input("stf", seed=41)

        def fresh(pattern):
            with _env(STF_PLAN="0"):
                n = _model("stf")
                n.load_state_dict(m.state_dict())
                _freeze(n, pattern)
                _step(n, x)
            return {k: p.grad for k, p in n.named_parameters()}
        # unfreeze: a new signature (eager warm step, then recorded, then replayed)
        m.requires_grad_(True)
        want = fresh(())
        for i in range(3):
            m.zero_grad(set_to_none=True)
            _step(m, x)
            for k, p in m.named_parameters():
                assert torch.equal(p.grad, want[k]), (i, k)
        assert rt.cur is not frozen_entry and rt.cur.bwd is not None
        # freeze again: back on the frozen plan
        _freeze(m, STF_ENC)
        want = fresh(STF_ENC)
        m.zero_grad(set_to_none=True)
        _step(m, x)
        assert rt.cur is frozen_entry
        for k, p in m.named_parameters():
            assert (p.grad is None and want[k] is None) or torch.equal(p.grad, want[k]), k


def test_frozen_step_peak_memory():
    """Eager steps at 64x64, B=4, T=4: the frozen-encoder step keeps no encoder intermediates for a
    backward that will not run, so its peak allocation is strictly below the all-trainable step's."""
    from stfunet import STFLSTMUNet
    from stfunet.synthetic import dce_batch
    x = dce_batch(4, 4, 64, 64, seed=3, device=DEV)[0]
    peak = {}
    with _env(STF_PLAN="0"):
        for name, pattern in (("all", ()), ("frozen", STF_ENC)):
            torch.manual_seed(0)
            m = _freeze(STFLSTMUNet(time_steps=4).to(DEV).train(), pattern)
            for measured in (False, True):            # (a first step settles packs and workspaces)
                m.zero_grad(set_to_none=True)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                m(x)["out"].square().mean().backward()
                torch.cuda.synchronize()
                peak[name] = torch.cuda.max_memory_allocated() - base
            del m
    print(f"\npeak allocated above the resident model: all-trainable {peak['all']} B, frozen encoder "
          f"{peak['frozen']} B")
    assert peak["frozen"] < peak["all"], peak


# ------------------------------------------------------------------ submodule modes
def _bn_state(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()
            if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


def _is_encoder(key):
    return key.startswith(("bn1.", "layer"))


def _randomize_running(m, seed):
    gen = torch.Generator().manual_seed(seed)
    sd = m.state_dict()
    for k, v in sd.items():
        if "running_mean" in k:
            sd[k] = torch.rand(v.shape, generator=gen) * 0.2 - 0.1
        if "running_var" in k:
            sd[k] = torch.rand(v.shape, generator=gen) * 0.5 + 0.75
    m.load_state_dict(sd)


def test_encoder_in_eval_keeps_its_statistics():
    """model.train() with the encoder submodules in .eval(): two training steps (one eager, then through
    the plan runtime's warm / record steps) leave every encoder running_mean / running_var /
    num_batches_tracked bit-unchanged while the decoder's advance."""
    batches = _batches(2, seed=760)
    m = _model("stf")
    _randomize_running(m, 3)
    _freeze(m, STF_ENC)
    for n in STF_ENC:
        m.get_submodule(n).eval()
    before = _bn_state(m)
    _train(m, [p for p in m.parameters() if p.requires_grad], 3, batches)
    after = _bn_state(m)
    n_enc = n_dec = 0
    for k in before:
        if _is_encoder(k):
            n_enc += 1
            assert torch.equal(before[k], after[k]), k
        else:
            n_dec += 1
            assert not torch.equal(before[k], after[k]), k
            if k.endswith("num_batches_tracked"):
                assert int(after[k]) == int(before[k]) + 3, k
    assert n_enc == 3 * (1 + 2 * 16 + 3) and n_dec == 3 * 8


def test_mixed_mode_logits_vs_oracle(monkeypatch):
    """Encoder in eval mode inside a training model: logits against a mixed-mode fp32 restatement
    composed from the oracle's own pieces (encoder with running statistics, LSTMs, decoder and head in
    training mode).  Metric and bound are the train-mode rule test_stf_gpu.py applies to whole-model
    logits at sizes not divisible by 32 (test_stf_size_fallback_train_vs_reference): rel L2 within
    1.3 x the bf16 emulation's error + 0.01, the emulation run in the same mixed mode."""
    import torch.nn.functional as F
    import oracle.unet_bf16 as o_q
    from oracle import stf as o_stf, stf_bf16 as o_emu
    from oracle.init import canonical_state_dict
    from stfunet import STFLSTMUNet
    from test_stf_gpu import rel
    m = STFLSTMUNet(in_channels=1, num_classes=2, time_steps=T)
    m.load_state_dict(canonical_state_dict(m.state_dict(), seed=0))
    _randomize_running(m, 5)
    sd = {k: v.clone().to(DEV) for k, v in m.state_dict().items()}
    m = m.to(DEV).train()
    for n in STF_ENC:
        m.get_submodule(n).eval()
    x = _input("stf", seed=12)

    def mixed(p):
        seqs = [[], [], [], []]
        for t in range(T):
            for s, e in zip(seqs, o_stf.encoder(x[:, t], p, training=False)):
                s.append(e)
        fused = []
        for i, s in enumerate(seqs, start=1):
            st = torch.stack(s, 1)
            bb, tt, cc, hh, ww = st.shape
            hT = o_stf.lstm_last_hidden(st.permute(0, 3, 4, 1, 2).reshape(bb * hh * ww, tt, cc), p, f"lstm{i}")
            fused.append(hT.reshape(bb, hh, ww, cc).permute(0, 3, 1, 2))
        e1, e2, e3, e4 = fused
        d = o_stf.decoder_block(e4, e3, p, "decoder4", training=True)
        d = o_stf.decoder_block(d, e2, p, "decoder3", training=True)
        d = o_stf.decoder_block(d, e1, p, "decoder2", training=True)
        d = F.conv_transpose2d(d, p["upconv1.weight"], p["upconv1.bias"], stride=2, padding=1, output_padding=1)
        d = o_stf.residual_conv_block(d, p, "final_res", training=True)
        return F.conv2d(d, p["final.weight"], p["final.bias"])
    with torch.no_grad():
        ref = mixed({k: v.clone() for k, v in sd.items()})
        # the bf16-storage emulation in the same mixed mode: its batch norms pick their mode by name
        bn = o_emu.batch_norm
        monkeypatch.setattr(o_emu, "batch_norm", lambda y, p, pre, tr: bn(y, p, pre, not _is_encoder(pre + ".")))
        with o_q.storage(torch.bfloat16):
            emu = o_emu.forward({k: v.clone() for k, v in sd.items()}, x, True)["out"]
        out = m(x)["out"]
    e_hip, e_emu = rel(out, ref), rel(emu, ref)
    print(f"\nmixed-mode logits rel {e_hip:.3e} (emulation {e_emu:.3e})")
    assert out.shape == ref.shape == (B, 2, H // 2, W // 2)
    assert e_hip <= 1.3 * e_emu + 0.01, (e_hip, e_emu)


@pytest.mark.parametrize("train", [True, False])
def test_uniform_modes_unchanged(train):
    """An all-train and an all-eval model behave as before: every BatchNorm advances (encoder T times,
    decoder once per forward) or none does."""
    m = _model("stf").train(train)
    before = _bn_state(m)
    with torch.no_grad():
        m(_input("stf"))
    torch.cuda.synchronize()
    after = _bn_state(m)
    for k in before:
        if not train:
            assert torch.equal(before[k], after[k]), k
        elif k.endswith("num_batches_tracked"):
            assert int(after[k]) == (T if _is_encoder(k) else 1), k
        else:
            assert not torch.equal(before[k], after[k]), k


# ------------------------------------------------------------------ optimizer
def test_adamw_one_launch_with_frozen_encoder():
    """AdamW over ``[p for p in model.parameters() if p.requires_grad]`` with the encoder frozen: the
    trainable set is a contiguous run of the flat order, so the step is ONE stf_adamw launch over the
    parameters in place (no gather / scatter of parameters, no gradient scratch copy)."""
    from stfunet.optim import AdamW
    m = _freeze(_model("stf"), STF_ENC)
    opt = AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    _step(m, _input("stf"))
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    with lt.tracing() as trace:
        opt.step()
        torch.cuda.synchronize()
    assert trace == ["stf_adamw"]
    fb = opt._flat[0]
    assert fb["p"] is not None and fb["gscratch"] is None
    assert fb["p"].data_ptr() == m.lstm1.weight_ih_l0.data_ptr()
    assert fb["n"] == m.program.flat.numel - m.program.flat.first_trainable_offset()
    for n, p in m.named_parameters():
        if not p.requires_grad:
            assert torch.equal(p, before[n]), n
        elif bool(p.grad.any()):                       # (a conv bias under a train-mode BN has gradient 0)
            assert not torch.equal(p, before[n]), n
