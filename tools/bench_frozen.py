"""Same-box interleaved A/B of the training step with the encoder frozen against the same step all
trainable: the cfg3-shape STF step (STFLSTMUNet, B = 16, T = 8, 256^2, bf16; conv1 / bn1 / layer1..4
frozen) and the cfg2 UNet step (UNet(in=8, base_c=64), B = 64, 256^2; enc1..4 frozen).  bench.py's step
(train_one_epoch's: forward, criterion, zero_grad, backward, AdamW over the parameters that require
grad, scheduler; the host reads the loss after every step), both models in one process, alternating
blocks of --steps steps for --rounds rounds after --warmup steps each (the plans record during the
warm-up).  The all-trainable side is the step as it was before freezing existed.

    python tools/bench_frozen.py [--models stf,unet] [--steps 20] [--rounds 6] [--warmup 10] [--out FILE]

Per model it prints per-round ms / step, then one JSON line: medians, each side's own spread
(max - min) / median over the rounds, the difference, ``torch.cuda.max_memory_allocated`` of each
side's timed blocks (planned steps keep every buffer of the recorded step alive, so the eager peak of
one extra step per side, STF_PLAN=0, is recorded too), and ``not_slower``: the frozen median is not
above the all-trainable median by more than the larger of the two spreads."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "stf-unet_amd")]
import torch  # noqa: E402
from stfunet import STFLSTMUNet, UNet, engine  # noqa: E402
from stfunet.optim import AdamW  # noqa: E402
from stfunet.synthetic import dce_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--models", default="stf,unet")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--time-steps", type=int, default=8)
ap.add_argument("--batch", type=int, default=None, help="default: 16 (stf), 64 (unet)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
FROZEN = {"stf": ("conv1", "bn1", "layer1", "layer2", "layer3", "layer4"), "unet": ("enc1", "enc2", "enc3", "enc4")}


def make(which, frozen):
    torch.manual_seed(1234)
    if which == "stf":
        model = STFLSTMUNet(in_channels=1, num_classes=2, time_steps=args.time_steps).to(dev)
    else:
        model = UNet(in_channels=args.time_steps, num_classes=2, base_c=64).to(dev)
    model.train()
    model.storage_dtype = torch.bfloat16
    if frozen:
        for name in FROZEN[which]:
            model.get_submodule(name).requires_grad_(False)
    opt = AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-4,
                eps=1e-8)
    sched = engine.create_lr_scheduler(opt, args.warmup + args.steps * args.rounds + 1, 10, warmup=True)
    batch = args.batch or (16 if which == "stf" else 64)
    half = (args.size // 2, args.size // 2) if which == "stf" else None
    batches = [dce_batch(batch, args.time_steps, args.size, args.size, seed=i, device=dev, mask_hw=half)
               for i in range(2)]
    batches = [(engine.preprocess_input(x, model), t) for x, t in batches]
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
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(k):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / k, torch.cuda.max_memory_allocated()


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


results = []
for which in args.models.split(","):
    sides = {"all": make(which, False), "frozen": make(which, True)}
    for step in sides.values():
        block(step, args.warmup)
    ms = {k: [] for k in sides}
    peak = {k: 0 for k in sides}
    for r in range(args.rounds):
        for k in (("all", "frozen") if r % 2 == 0 else ("frozen", "all")):
            t, pk = block(sides[k], args.steps)
            ms[k].append(t)
            peak[k] = max(peak[k], pk)
        print(f"{which} round {r}: all-trainable {ms['all'][-1]:.3f} ms/step, frozen encoder {ms['frozen'][-1]:.3f}",
              flush=True)
    eager_peak = {}
    os.environ["STF_PLAN"] = "0"
    for k, step in sides.items():
        eager_peak[k] = block(step, 1)[1]
    del os.environ["STF_PLAN"]
    med = {k: statistics.median(v) for k, v in ms.items()}
    sp = {k: spread(v) for k, v in ms.items()}
    res = dict(model=which, size=args.size, time_steps=args.time_steps, steps=args.steps, rounds=args.rounds,
               ms_all=med["all"], ms_frozen=med["frozen"], spread_all=sp["all"], spread_frozen=sp["frozen"],
               diff_pct=100.0 * (med["frozen"] - med["all"]) / med["all"],
               not_slower=med["frozen"] <= med["all"] * (1.0 + max(sp.values())),
               max_memory_allocated_all=peak["all"], max_memory_allocated_frozen=peak["frozen"],
               eager_max_memory_allocated_all=eager_peak["all"], eager_max_memory_allocated_frozen=eager_peak["frozen"],
               rounds_ms=ms)
    print(json.dumps(res), flush=True)
    results.append(res)
    del sides
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
if not all(r["not_slower"] for r in results):
    sys.exit("frozen step slower than the all-trainable step beyond the box's run-to-run spread")
