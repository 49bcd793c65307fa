"""Same-box interleaved timing of the optimizer step with and without gradient clipping, on the
gradients of a real backward: the cfg2-shape UNet (UNet(in=8, base_c=64), B = 64, 256^2; --batch and
--size shrink the backward, the gradient buffer's size does not depend on them) and the cfg3-shape STF
model (STFLSTMUNet, T = 8).  Four arms per model, each on the same gradient buffer, alternating for
--rounds rounds of --iters calls after --warmup calls:

  a  optimizer.step()                                          (the step as it is without clipping)
  b  AdamW(max_grad_norm=m).step()                             (stf_grad_norm + stf_adamw_clip)
  c  stfunet.optim.clip_grad_norm_(params, m); step()          (stf_grad_norm + stf_grad_scale + stf_adamw)
  d  torch.nn.utils.clip_grad_norm_(params, m); step()
  d_unscale (--fp16 only)  scaler.unscale_-style pass (torch._amp_foreach_non_finite_check_and_unscale_
     over the gradient views) + d, against b with a device grad_scale / found_inf

m is twice the measured norm, so no arm changes the gradients it times (a coefficient of 1: arm c's
scale kernel returns without writing, torch multiplies by 1.0); parameters drift with lr = 1e-6 only.
Per arm: GPU time event to event per call and host time per call (time until the call returns, no
synchronisation inside the timed region), median over the rounds.  The norm pass alone is timed too
(stf_grad_norm, both launches) and reported as bytes read per second.

    python tools/bench_clip.py [--models unet,stf] [--iters 20] [--rounds 7] [--out profiles/clip/clip.json]
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
from stfunet import STFLSTMUNet, UNet, engine  # noqa: E402
from stfunet import optim as so  # noqa: E402
from stfunet.synthetic import dce_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--models", default="unet,stf")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--batch", type=int, default=None, help="default: 64 (unet), 16 (stf)")
ap.add_argument("--fp16", action="store_true", help="fp16 storage; adds the GradScaler arms")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)


def make(which):
    torch.manual_seed(1234)
    model = (UNet(in_channels=8, num_classes=2, base_c=64) if which == "unet" else
             STFLSTMUNet(in_channels=1, num_classes=2, time_steps=8)).to(dev).train()
    model.storage_dtype = torch.float16 if args.fp16 else torch.bfloat16
    batch = args.batch or (64 if which == "unet" else 16)
    half = (args.size // 2, args.size // 2) if which == "stf" else None
    x, t = dce_batch(batch, 8, args.size, args.size, seed=0, device=dev, mask_hw=half)
    os.environ["STF_PLAN"] = "0"
    engine.criterion(model(engine.preprocess_input(x, model)), t).backward()
    del os.environ["STF_PLAN"]
    torch.cuda.synchronize()
    return model


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


results = []
for which in args.models.split(","):
    model = make(which)
    params = list(model.parameters())
    norm = float(torch.nn.utils.get_total_norm([p.grad for p in params])) if hasattr(torch.nn.utils, "get_total_norm") \
        else float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in params)))
    m = 2.0 * norm
    kw = dict(lr=1e-6, weight_decay=1e-4)
    plain, fused = so.AdamW(params, **kw), so.AdamW(params, max_grad_norm=m, **kw)
    arms = {
        "a": plain.step,
        "b": fused.step,
        "c": lambda: (so.clip_grad_norm_(params, m), plain.step()),
        "d": lambda: (torch.nn.utils.clip_grad_norm_(params, m), plain.step()),
    }
    if args.fp16:
        scale = torch.full((), 1.0, device=dev)          # a scale of 1: the passes run, the values stay
        inv, finf = scale.reciprocal(), torch.zeros((), device=dev)
        grads = [p.grad for p in params]

        def b_amp():
            fused.grad_scale, fused.found_inf = scale, finf
            fused.step()
            del fused.grad_scale, fused.found_inf

        def d_unscale():
            torch._amp_foreach_non_finite_check_and_unscale_(grads, finf, inv)
            torch.nn.utils.clip_grad_norm_(params, m)
            plain.step()
        arms["b_amp"], arms["d_unscale"] = b_amp, d_unscale
    table = fused._clip_table(params, fused._group_buffers(0, fused.param_groups[0]))
    flat = fused._flat_grad(params, fused._flat[0])
    arms["norm_only"] = lambda: so._grad_norm(flat, table, m)
    for fn in arms.values():
        timed(fn, args.warmup)
    gpu, host = {k: [] for k in arms}, {k: [] for k in arms}
    order = list(arms)
    for r in range(args.rounds):
        for k in (order if r % 2 == 0 else order[::-1]):
            g, h = timed(arms[k], args.iters)
            gpu[k].append(g)
            host[k].append(h)
        print(f"{which} round {r}: " + "  ".join(f"{k} {gpu[k][-1] * 1e3:.1f}" for k in order) + "  (GPU us/call)",
              flush=True)
    med = {k: statistics.median(v) for k, v in gpu.items()}
    nbytes = 4 * table.total
    res = dict(model=which, storage="fp16" if args.fp16 else "bf16", parameters=len(params), elements=table.total,
               segments=table.count, grad_norm=norm, iters=args.iters, rounds=args.rounds,
               gpu_us={k: 1e3 * med[k] for k in order},
               gpu_spread={k: (max(v) - min(v)) / statistics.median(v) for k, v in gpu.items()},
               host_us={k: 1e3 * statistics.median(v) for k, v in host.items()},
               norm_pass_bytes=nbytes, norm_pass_TBps=nbytes / (med["norm_only"] * 1e-3) / 1e12,
               rounds_gpu_ms=gpu)
    print(json.dumps(res), flush=True)
    results.append(res)
    del model, params, plain, fused, arms
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
