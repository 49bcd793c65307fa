"""Logits-resize kernel pair timing (stf_resize_bilinear_fwd + stf_resize_bilinear_bwd) at the cfg3
logits shape (16 x 2 x 128^2 -> 256^2) and at 16 classes, beside torch's F.interpolate forward +
backward on the same device as the reference point; interleaved in one process, HIP events over
--reps launches per round after warm-up (the method of tools/bench_loss.py).

    python tools/bench_resize.py [--reps 200] [--rounds 7] [--shapes 16,2,128,256;16,16,128,256] [--out FILE]

One JSON line per shape: us per launch (median and min over the rounds) and effective GB/s on the
algorithmic bytes (4 (h w + H W) per plane for either direction: every element read or written once)
for the forward, the backward and the pair, the same for torch's forward and backward, and the
ratios.  The gradients of the two are compared once (max abs difference) before timing."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "stf-unet_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from stfunet import _lib  # noqa: E402
from stfunet._lib import stream  # noqa: E402
from stfunet.nhwc import _p  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--shapes", default="16,2,128,256;16,16,128,256", help="N,K,low,high per shape, ';' between shapes")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = "cuda"
lib = _lib.load()


def timeit(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.reps * 1e3     # us per call


def check(rc):
    if rc != 0:
        raise RuntimeError(f"launch failed: {rc}")


def one_shape(N, K, lo, hi):
    gen = torch.Generator(device=dev).manual_seed(K)
    x = torch.randn(N, K, lo, lo, device=dev, generator=gen) * 2
    dy = torch.randn(N, K, hi, hi, device=dev, generator=gen)
    y, dx = torch.empty_like(dy), torch.empty_like(x)
    xt = x.clone().requires_grad_(True)
    planes = N * K
    nbytes = 4 * planes * (lo * lo + hi * hi)

    def fwd():
        check(lib.stf_resize_bilinear_fwd(_p(x), planes, lo, lo, _p(y), hi, hi, stream()))

    def bwd():
        check(lib.stf_resize_bilinear_bwd(_p(dy), planes, hi, hi, _p(dx), lo, lo, stream()))

    state = {}

    def torch_fwd():
        state["y"] = F.interpolate(xt, size=(hi, hi), mode="bilinear", align_corners=False)

    def torch_bwd():                         # (on the graph of the last torch_fwd)
        xt.grad = None
        state["y"].backward(dy, retain_graph=True)

    fns = {"fwd": fwd, "bwd": bwd, "torch_fwd": torch_fwd, "torch_bwd": torch_bwd}
    for fn in fns.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    diff = {"fwd_max_abs_diff": (y - state["y"].detach()).abs().max().item(),
            "bwd_max_abs_diff": (dx - xt.grad).abs().max().item()}
    times = {k: [] for k in fns}
    for r in range(args.rounds):
        for k, fn in fns.items():
            times[k].append(timeit(fn))
        print(f"{N}x{K}x{lo}^2->{hi}^2 round {r}: " + "   ".join(f"{k} {v[-1]:7.2f} us" for k, v in times.items()),
              flush=True)
    res = {"shape": [N, K, lo, hi], "reps": args.reps, "rounds": args.rounds, "bytes": nbytes, **diff}
    for k, v in times.items():
        m = statistics.median(v)
        res[k] = {"median_us": m, "min_us": min(v), "spread": (max(v) - min(v)) / m, "GBps": nbytes / m * 1e-3}
    pair = [a + b for a, b in zip(times["fwd"], times["bwd"])]
    tpair = [a + b for a, b in zip(times["torch_fwd"], times["torch_bwd"])]
    res["pair_us"] = {"median": statistics.median(pair), "min": min(pair)}
    res["torch_pair_us"] = {"median": statistics.median(tpair), "min": min(tpair)}
    res["pair_over_torch"] = res["pair_us"]["median"] / res["torch_pair_us"]["median"]
    return res


lines = [json.dumps(one_shape(*(int(v) for v in s.split(",")))) for s in args.shapes.split(";")]
print("\n".join(lines))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
