"""Same-box interleaved A/B of the cfg3 training step (STFLSTMUNet, B = 16, T = 8, 256^2, bf16) with
``output_size="half"`` against ``output_size="input"``: bench.py's step (train_one_epoch's: forward,
criterion, zero_grad, backward, AdamW, scheduler; the host reads the loss after every step), both
models in one process, alternating blocks of --steps steps for --rounds rounds after --warmup steps
each (the plans record during the warm-up).

    python tools/ab_output_size.py [--steps 20] [--rounds 6] [--warmup 10] [--out FILE]

"half" trains against half-resolution masks (bench.py's ``mask_hw``), "input" against the
full-resolution ones, so "input" carries the resize pair AND a criterion over 4x the pixels.  Prints
per-round ms / step, then one JSON line: medians, each side's own spread (max - min) / median over
the rounds, and the difference."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "stf-unet_amd")]
import torch  # noqa: E402
from stfunet import STFLSTMUNet, engine  # noqa: E402
from stfunet.optim import AdamW  # noqa: E402
from stfunet.synthetic import dce_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--time-steps", type=int, default=8)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)


def make(output_size):
    torch.manual_seed(1234)
    model = STFLSTMUNet(in_channels=1, num_classes=2, time_steps=args.time_steps, output_size=output_size).to(dev)
    model.train()
    model.storage_dtype = torch.bfloat16
    opt = AdamW(model.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-4, eps=1e-8)
    sched = engine.create_lr_scheduler(opt, args.warmup + args.steps * args.rounds, 10, warmup=True)
    half = (args.size // 2, args.size // 2) if output_size == "half" else None
    batches = [dce_batch(args.batch, args.time_steps, args.size, args.size, seed=i, device=dev, mask_hw=half)
               for i in range(2)]
    n = [0]

    def step():
        x, t = batches[n[0] % 2]
        n[0] += 1
        loss = engine.criterion(model(x), t)
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
        return loss.item()
    return step


def block(step, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


steps = {name: make(name) for name in ("half", "input")}
for s in steps.values():
    block(s, args.warmup)
times = {name: [] for name in steps}
for r in range(args.rounds):
    for name, s in steps.items():
        times[name].append(block(s, args.steps))
    print(f"round {r}: " + "   ".join(f"{k} {v[-1]:8.3f} ms/step" for k, v in times.items()), flush=True)
res = {"workload": f"STF B{args.batch} T{args.time_steps} {args.size}^2 bf16", "steps": args.steps, "rounds": args.rounds}
for name, v in times.items():
    m = statistics.median(v)
    res[name] = {"median_ms": m, "min_ms": min(v), "spread": (max(v) - min(v)) / m}
res["input_minus_half_ms"] = res["input"]["median_ms"] - res["half"]["median_ms"]
res["input_over_half"] = res["input"]["median_ms"] / res["half"]["median_ms"]
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
