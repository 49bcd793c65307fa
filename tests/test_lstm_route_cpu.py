"""The LSTM route (stfunet/stf_lstm_unet.py: LstmRoute, lstm_route) on the CPU: which launches run
an LSTM is resolved by one pure function of the hidden size and the buffer layout (the library is
asked which sizes its kernels take; nothing is launched), and no environment variable steers it."""
import glob
import os

import pytest

from conftest import REPO

# lstm1-4 at cfg3: hidden size, channel stride of the h_T destination (the decoder's concat buffer
# for lstm1-3, whose skip half starts at channel C; a dense buffer for lstm4)
CFG3 = [(64, 128), (128, 256), (256, 512), (512, 512)]


def test_default_and_forced_lstm_routes():
    from stfunet.stf_lstm_unet import LSTM_COOP, LstmRoute, lstm_route
    assert LSTM_COOP == frozenset({512})
    want = {64: LstmRoute("seq", "seq"), 128: LstmRoute("step", "recompute", True),
            256: LstmRoute("step", "recompute", True), 512: LstmRoute("coop", "gates", True)}
    for C, hcs in CFG3:
        assert lstm_route(C, 0, 2 * C, hcs, 0) == want[C], C
    assert lstm_route(64, 0, 128, 128, 0)[:2] == ("seq", "seq")
    # no backward: the cooperative forward keeps no gates
    assert lstm_route(512, 0, 1024, 512, 0, need_bwd=False) == LstmRoute("coop", "recompute", True)
    assert lstm_route(64, 0, 128, 128, 0, need_bwd=False) == LstmRoute("seq", "seq")
    # the program's cooperative set: every supported size, none, and a size no kernel takes
    every = frozenset({64, 128, 256, 512})
    assert [lstm_route(C, 0, 2 * C, hcs, 0, coop=every).fwd for C, hcs in CFG3] == ["seq", "coop", "coop", "coop"]
    assert [lstm_route(C, 0, 2 * C, hcs, 0, coop=frozenset()).fwd for C, hcs in CFG3] == ["seq", "step", "step",
                                                                                           "step"]
    assert lstm_route(32, 0, 64, 32, 0, coop=frozenset({32})) == LstmRoute("step", "recompute", True)
    # layouts the whole-sequence kernels do not take fall back to the per-step launches
    step = LstmRoute("step", "recompute", True)
    assert lstm_route(512, 0, 1024, 516, 0) == step                 # hT.cs % 8 != 0
    assert lstm_route(512, 0, 1024, 512, 8) == step                 # hT not 16-byte aligned
    assert lstm_route(512, 0, 1024 + 8, 512, 0) == step             # [x | h] rows not packed
    assert lstm_route(64, 8, 128, 128, 0) == step                   # lbuf.off != 0
    assert lstm_route(64, 0, 128, 56, 0) == step                    # hT narrower than C
    # forced routes: returned as given where this C and layout can run them ...
    for C, hcs in CFG3:
        for hoist in (False, True):
            r = LstmRoute("step", "recompute", hoist)
            assert lstm_route(C, 0, 2 * C, hcs, 0, forced=r) == r
            if C > 64:
                for bwd in ("gates", "recompute"):
                    r = LstmRoute("coop", bwd, hoist)
                    assert lstm_route(C, 0, 2 * C, hcs, 0, coop=frozenset(), forced=r) == r
    # ("seq" has no hoist: one value, so that routes compare equal)
    assert lstm_route(64, 0, 128, 128, 0, forced=LstmRoute("seq", "seq", False)) == LstmRoute("seq", "seq")
    # ... and ValueError where they cannot, at resolution time
    bad = [(64, 0, 128, 128, 0, LstmRoute("step", "gates", True)),        # gates without a coop forward
           (64, 0, 128, 128, 0, LstmRoute("seq", "gates", True)),
           (128, 0, 256, 256, 0, LstmRoute("seq", "seq", True)),          # seq at an unsupported C
           (64, 8, 128, 128, 0, LstmRoute("seq", "seq", True)),           # ... or layout
           (64, 0, 128, 128, 0, LstmRoute("coop", "gates", True)),        # coop at an unsupported C
           (512, 0, 1024, 516, 0, LstmRoute("coop", "gates", True)),      # ... or layout
           (512, 0, 1024, 512, 8, LstmRoute("coop", "recompute", True)),
           (64, 0, 128, 128, 0, LstmRoute("seq", "recompute", True)),     # seq forward and backward go together
           (512, 0, 1024, 512, 0, LstmRoute("coop", "seq", True)),
           (64, 0, 128, 128, 0, LstmRoute("fused", "seq", True)),         # no such route
           (64, 0, 128, 128, 0, LstmRoute("step", "coop", True))]
    for C, off, cs, hcs, ptr, r in bad:
        with pytest.raises(ValueError):
            lstm_route(C, off, cs, hcs, ptr, forced=r)


def test_route_overrides_are_plan_knobs():
    """A recorded plan carries the routes by value: a changed ``route`` / ``lstm_coop`` is a new signature."""
    from stfunet import STFLSTMUNet
    from stfunet.stf_lstm_unet import LstmRoute
    p = STFLSTMUNet(time_steps=2).program
    assert p.lstm_coop == frozenset({512}) and [lp.route for lp in p.lstm_progs] == [None] * 4
    assert [lp.max_wg for lp in p.lstm_progs] == [64, 64, 64, 0]
    k0 = p.plan_knobs()
    hash(k0)
    p.lstm_coop = frozenset()
    k1 = p.plan_knobs()
    p.lstm_coop = frozenset({512})
    p.lstm_progs[3].route = LstmRoute("step", "recompute", False)
    k2 = p.plan_knobs()
    p.lstm_progs[3].route = None
    assert len({k0, k1, k2}) == 3 and p.plan_knobs() == k0


RETIRED = ("STF_LSTM_SEQ", "STF_LSTM_COOP", "STF_LSTM_COOP_BWD", "STF_LSTM_HOIST", "STF_LSTM_GATES",
           "STF_LSTM_SIDE_WG", "STF_SIDE_STREAMS")


def test_retired_lstm_knobs_are_not_read():
    """The seven environment variables that used to steer the LSTM are named nowhere in the package."""
    files = sorted(glob.glob(os.path.join(REPO, "stf-unet_amd", "stfunet", "*.py")))
    assert len(files) > 10
    for f in files:
        src = open(f).read()
        for name in RETIRED:
            assert name not in src, (os.path.basename(f), name)
