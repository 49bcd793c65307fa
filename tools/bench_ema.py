"""Same-box interleaved measurements of the weight EMA (stfunet.WeightEMA), three sets of figures.

  kernels   stf_ema_update and stf_ema_swap on the table of the cfg2 UNet (UNet(in=8, base_c=64):
            31,046,466 parameters plus its BatchNorm buffers) and of the cfg3 STF model
            (STFLSTMUNet, T = 8), and stf_adamw over the same flat parameter buffer as the yardstick
            (28 B per element: p, g, m, v read, p, m, v written).  Arms alternate for --rounds rounds
            of --iters calls; per arm the median GPU time event to event and the achieved bytes/s
            (update 12 B, swap 16 B per element).  Acceptance: the update's bytes/s is not lower than
            AdamW's by more than the spread (max - min over the rounds) of the AdamW measurement itself.
  step      the cfg2 training step (B = 64, 256^2; --batch / --size shrink it) with and without
            ema.update(), alternating blocks on one model.  Recorded, not gated.
  bolt-on   torch.optim.swa_utils.AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(d),
            use_buffers=True) on the same model: time per update_parameters against ema.update(), and
            the device memory each holds (the bolt-on once its copy has run an eval forward).

    python tools/bench_ema.py [--models unet,stf] [--iters 20] [--rounds 7] [--out profiles/ema/ema.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "stf-unet_amd")]
import torch  # noqa: E402
from stfunet import STFLSTMUNet, UNet, WeightEMA, engine  # noqa: E402
from stfunet import optim as so  # noqa: E402
from stfunet._lib import call, stream  # noqa: E402
from stfunet.nhwc import _p  # noqa: E402
from stfunet.synthetic import dce_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--models", default="unet,stf")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--step-iters", type=int, default=10)
ap.add_argument("--skip-step", action="store_true")
ap.add_argument("--skip-bolt-on", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)


def make(which):
    torch.manual_seed(1234)
    return (UNet(in_channels=8, num_classes=2, base_c=64) if which == "unet" else
            STFLSTMUNet(in_channels=1, num_classes=2, time_steps=8)).to(dev).train()


def timed(fn, k):
    """(GPU ms per call, event to event; host ms per call) of k calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    host = (time.perf_counter() - t0) * 1e3 / k
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / k, host


def interleaved(arms, iters, rounds, warmup, label):
    for fn in arms.values():
        timed(fn, warmup)
    gpu, host = {k: [] for k in arms}, {k: [] for k in arms}
    order = list(arms)
    for r in range(rounds):
        for k in (order if r % 2 == 0 else order[::-1]):
            g, h = timed(arms[k], iters)
            gpu[k].append(g)
            host[k].append(h)
        print(f"{label} round {r}: " + "  ".join(f"{k} {gpu[k][-1] * 1e3:.1f}" for k in order) + "  (GPU us/call)",
              flush=True)
    return gpu, host


def kernel_rates(which):
    model = make(which)
    ema = WeightEMA(model, decay=0.999)
    ema.update()                                         # the copy; from here on w = 0.001
    flat = model.program.flat
    n = flat.numel
    g, m, v = (torch.zeros(n, dtype=torch.float32, device=dev) for _ in range(3))
    elements = sum(s[2] for s in ema.layout.segs)
    t = ema._tab()

    def update():
        call("stf_ema_update", ema.shadow.data_ptr(), t.dptr, t.hptr, t.count, 0.001, stream())

    def swap():
        call("stf_ema_swap", ema.shadow.data_ptr(), t.dptr, t.hptr, t.count, stream())

    def adamw():                                         # lr = 0, no decay: the parameters stay
        call("stf_adamw", _p(flat.data), _p(g), _p(m), _p(v), n, 0.0, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, stream())

    arms = {"update": update, "swap": swap, "adamw": adamw}
    nbytes = {"update": 12 * elements, "swap": 16 * elements, "adamw": 28 * n}
    gpu, host = interleaved(arms, args.iters, args.rounds, args.warmup, f"{which} kernels")
    med = {k: statistics.median(x) for k, x in gpu.items()}
    rate = {k: nbytes[k] / (med[k] * 1e-3) / 1e9 for k in arms}
    per_round = {k: [nbytes[k] / (x * 1e-3) / 1e9 for x in gpu[k]] for k in arms}
    spread = max(per_round["adamw"]) - min(per_round["adamw"])
    res = dict(set="kernels", model=which, parameters=len(flat.params), flat_elements=n, table_elements=elements,
               segments=t.count, iters=args.iters, rounds=len(gpu["adamw"]),
               gpu_us={k: 1e3 * med[k] for k in arms}, host_us={k: 1e3 * statistics.median(x) for k, x in host.items()},
               bytes=nbytes, GBps=rate, GBps_rounds=per_round, adamw_spread_GBps=spread,
               update_minus_adamw_GBps=rate["update"] - rate["adamw"],
               accepted=bool(rate["update"] >= rate["adamw"] - spread))
    del model, ema, g, m, v
    torch.cuda.empty_cache()
    return res


def step_cost():
    model = make("unet")
    x, t = dce_batch(args.batch, 8, args.size, args.size, seed=0, device=dev)
    x = engine.preprocess_input(x, model)
    opt = so.AdamW(model.parameters(), lr=1e-6, weight_decay=1e-4)
    ema = WeightEMA(model, decay=0.999)

    def step():
        loss = engine.criterion(model(x), t)
        opt.zero_grad()
        loss.backward()
        opt.step()

    def step_ema():
        step()
        ema.update()

    arms = {"step": step, "step_ema": step_ema}
    gpu, host = interleaved(arms, args.step_iters, args.rounds, args.warmup, "cfg2 step")
    med = {k: statistics.median(v) for k, v in gpu.items()}
    res = dict(set="step", model="unet", batch=args.batch, size=args.size, iters=args.step_iters, rounds=args.rounds,
               gpu_ms=med, gpu_spread={k: (max(v) - min(v)) / statistics.median(v) for k, v in gpu.items()},
               host_ms={k: statistics.median(v) for k, v in host.items()},
               ema_cost_ms=med["step_ema"] - med["step"], rounds_gpu_ms=gpu)
    del model, opt, ema
    torch.cuda.empty_cache()
    return res


def bolt_on():
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    model = make("unet")
    x, _ = dce_batch(2, 8, 64, 64, seed=0, device=dev)
    x = engine.preprocess_input(x, model)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    # the copy is taken from a model that has not run yet: deepcopy refuses a model whose program
    # holds a freeze map (FreezeMap is immutable), i.e. any model after its first training forward
    avg = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(0.999), use_buffers=True)
    avg.update_parameters(model)
    with torch.no_grad():
        avg.module.eval()(x)
    torch.cuda.synchronize()
    mem_bolt = torch.cuda.memory_allocated() - base
    with torch.no_grad():
        model.eval()(x)
        model.train()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    ema = WeightEMA(model, decay=0.999)
    ema.update()
    with torch.no_grad(), ema.averaged():
        model.eval()(x)
        model.train()
    torch.cuda.synchronize()
    mem_native = torch.cuda.memory_allocated() - base
    arms = {"native": ema.update, "bolt_on": lambda: avg.update_parameters(model)}
    gpu, host = interleaved(arms, args.iters, args.rounds, args.warmup, "bolt-on")
    return dict(set="bolt_on", model="unet", iters=args.iters, rounds=args.rounds,
                gpu_us={k: 1e3 * statistics.median(v) for k, v in gpu.items()},
                host_us={k: 1e3 * statistics.median(v) for k, v in host.items()},
                memory_bytes={"native": mem_native, "bolt_on": mem_bolt}, rounds_gpu_ms=gpu)


results = []


def keep(res):
    """Print the set's line and rewrite --out with everything measured so far."""
    results.append(res)
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


for which in args.models.split(","):
    keep(kernel_rates(which))
if not args.skip_step:
    keep(step_cost())
if not args.skip_bolt_on:
    keep(bolt_on())
