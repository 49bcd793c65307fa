"""Cases and digests of tests/golden/loss_bits.json and loss_bits_manyclass.json (shared by their
generator and their test).

Every case is a seed and a shape; the inputs come from ``numpy.random.default_rng(seed)``.  A
family is one pair of C entry points with one option set; ``digests`` runs forward then backward
through them and returns the SHA-256 of the raw bytes of the loss, of the documented leading
floats of ``terms`` and of ``dlogits`` (pre-filled with NaN, so an unwritten element shows).
"""
import hashlib

import numpy as np
import torch

IGNORE = 255
GRAD_OUT = 0.75

# (N, K, H, W): the smallest shape that reaches each seam of the three kernels
SHAPES = [(2, 2, 136, 136),     # HW > 64 * 256: the forward's chunk loop takes a second trip
          (65, 2, 8, 8),        # the finalize's second block of 64 images
          (3, 4, 16, 24),
          (2, 1, 16, 16),
          (2, 3, 16, 16),       # with the three above: every K of the dispatch
          (33, 2, 256, 256)]    # N * HW > 8192 * 256: the backward's grid-stride loop, second trip
FAMILIES = {"default": None, "option": 1, "option_nodice": 0}      # name -> the dice argument


# loss_bits_manyclass.json: the many-class (stf_loss_mc_*) and focal / Tversky (stf_loss_ft_*) entry points.
# name -> (entry-point infix, the dice argument, (gamma, alpha, beta) or ())
MC_FAMILIES = {"mc": ("mc", 1, ()), "mc_nodice": ("mc", 0, ()),
               "ft": ("ft", 1, (2.0, 0.3, 0.7)), "ft_tversky_only": ("ft", 1, (0.0, 0.3, 0.7)),
               "ft_focal_nodice": ("ft", 0, (0.5, 0.5, 0.5))}
MC_SHAPES = [((2, 7, 136, 136), ("mc", "ft")),      # the forward's second, ragged chunk trip; KP = 8 with K < KP
             ((65, 5, 8, 8), ("mc", "ft")),         # the finalize's second block of 64 images
             ((3, 16, 16, 24), ("mc", "ft")),       # KP = 16 full
             ((3, 9, 16, 24), ("mc", "ft")),        # KP = 16 ragged
             ((33, 5, 256, 256), ("mc",)),          # 8192 / 33 = 248 blocks of 256 threads < HW: the backward's
             ((33, 2, 256, 256), ("ft",)),          # grid-stride loop takes a second trip
             ((2, 1, 16, 16), ("ft",)),             # K = 1 in KP = 4
             ((2, 3, 16, 16), ("ft",)),             # K = 3 in KP = 4
             ((2, 4, 16, 16), ("mc",)),             # KP = 4 full (a direct call: legal for the C entry point)
             ((3, 7, 24, 16), ("mc_nodice", "ft_tversky_only", "ft_focal_nodice"))]


def cases():
    out = [(f, s) for s in SHAPES for f in ("default", "option")]
    out.append(("option_nodice", (3, 4, 16, 24)))
    return out


def mc_cases():
    return [(f, s) for s, fams in MC_SHAPES for f in fams]


def case_id(family, shape):
    return f"{family}-" + "x".join(str(v) for v in shape)


def seed_of(shape):
    N, K, H, W = shape
    return 100000 * N + 10000 * K + 100 * H + W


def inputs(family, shape):
    """logits [N, K, H, W] fp32, target [N, H, W] int64, class weights (None for the default family).
    The option families pad a band of columns of the first image and a band of rows of the last
    with 255 and ignore one whole image."""
    N, K, H, W = shape
    rng = np.random.default_rng(seed_of(shape))
    logits = (rng.standard_normal((N, K, H, W)) * 3.0).astype(np.float32)
    target = rng.integers(0, K, (N, H, W), dtype=np.int64)
    if family == "default":
        return logits, target, None
    target[0, :, W - max(1, W // 4):] = IGNORE
    target[-1, H - max(1, H // 4):, :] = IGNORE
    target[N // 2] = IGNORE
    return logits, target, np.array([0.5 + 0.75 * k for k in range(K)], dtype=np.float32)


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def digests(family, shape, dev="cuda"):
    from stfunet import _lib
    from stfunet._lib import call, stream
    from stfunet.nhwc import _p
    N, K, H, W = shape
    logits, target, weight = inputs(family, shape)
    x, t = torch.from_numpy(logits).to(dev), torch.from_numpy(target).to(dev)
    loss = torch.full((1,), float("nan"), device=dev)
    go = torch.full((1,), GRAD_OUT, device=dev)
    dl = torch.full_like(x, float("nan"))
    lib = _lib.load()
    if family == "default":
        terms = torch.zeros(lib.stf_loss_scratch_floats(N, K), device=dev)
        lead = N * K * 3 + 1
        call("stf_loss_fwd", _p(x), _p(t), N, H, W, K, _p(terms), _p(loss), stream())
        call("stf_loss_bwd", _p(x), _p(t), N, H, W, K, _p(terms), _p(go), _p(dl), stream())
    elif family in MC_FAMILIES:
        ep, dice, ft = MC_FAMILIES[family]
        w = torch.from_numpy(weight).to(dev)
        terms = torch.zeros(getattr(lib, f"stf_loss_{ep}_scratch_floats")(N, K), device=dev)
        lead = N * K * 3 + 2
        opts = (_p(w), IGNORE, dice, *ft)
        call(f"stf_loss_{ep}_fwd", _p(x), _p(t), N, H, W, K, *opts, _p(terms), _p(loss), stream())
        call(f"stf_loss_{ep}_bwd", _p(x), _p(t), N, H, W, K, *opts, _p(terms), _p(go), _p(dl), stream())
    else:
        dice = FAMILIES[family]
        w = torch.from_numpy(weight).to(dev)
        terms = torch.zeros(lib.stf_loss_opt_scratch_floats(N, K), device=dev)
        lead = N * K * 3 + 2
        call("stf_loss_opt_fwd", _p(x), _p(t), N, H, W, K, _p(w), IGNORE, dice, _p(terms), _p(loss), stream())
        call("stf_loss_opt_bwd", _p(x), _p(t), N, H, W, K, _p(w), IGNORE, dice, _p(terms), _p(go), _p(dl),
             stream())
    torch.cuda.synchronize()
    return {"loss": _sha(loss), "terms": _sha(terms[:lead]), "dlogits": _sha(dl), "loss_value": float(loss[0])}
