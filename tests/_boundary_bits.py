"""Cases and digests of tests/golden/boundary_bits.json (shared by its generator and its test).

Every case is a name, a shape and a seed; the inputs come from ``numpy.random.default_rng(seed)``.
``digests`` calls the C entry points of csrc/boundary.hip and csrc/bloss.hip directly and returns the
SHA-256 of the raw bytes of every output, and the scratch byte count of the shape.  Outputs are
pre-filled with 0xAA bytes (NaN where the entry point accumulates into them would hide the result, so
those get a fixed pattern), the scratch with 0xAA as well: an element that is not written shows.

Each shape is the smallest that reaches one seam of the kernels (the comments name it).
"""
import hashlib

import numpy as np
import torch

IGNORE = 255
GRAD_OUT = 0.75
ALPHA = 0.5

# images (B, H, W)
IMAGES = {
    "img-3x40x65": (3, 40, 65),       # a word seam at 64; HW = 2600 > 2 * 1024: the fold's strided loop takes a
                                      # third, ragged trip; `where` mask and an ignore band
    "img-1x1x4096": (1, 1, 4096),     # 64 words, H = 1, d2 up to 4095^2: every bin of the first radix digit
    "img-2x300x3": (2, 300, 3),       # long column scans, W < 64; the second image is empty (NaN, INT32_MAX)
}
# volumes (N, H, W), depths, spacing rows (one per volume)
_EXACT = [(1.0, 1.0, 1.0), (2.5, 0.75, 0.75), (3.0, 0.5, 0.625)]
VOLUMES = {
    # HW = 2600 > 2048: two units per slice and side, the second ragged; the last volume has no prediction
    "vol-6x40x65-unit": ((6, 40, 65), (1, 3, 2), [(1.0, 1.0, 1.0)] * 3),
    "vol-6x40x65-spaced": ((6, 40, 65), (1, 3, 2), _EXACT),
    # 66000 units > 65536 blocks: the depth kernel's block-stride loop takes a second trip
    "vol-33000x1x2": ((33000, 1, 2), (16500, 16500), [(1.0, 1.0, 1.0), (2.5, 0.75, 0.75)]),
    # both percentile ranks inside a run of equal values (volume 0) and the lower one on the run's last
    # element (volume 1): see _ties
    "vol-10x12x12-ties": ((10, 12, 12), (5, 5), [(1.0, 1.0, 1.0), (2.5, 0.75, 0.75)]),
}
# maps (N, K, H, W), K classes
MAPS = {
    "map-2x3x19x65": (2, 3, 19, 65),  # H = 2 * 8 + 3: ragged against the 8-row prefetch; a word seam
    "map-1x2x1x130": (1, 2, 1, 130),  # H = 1
    "map-2x2x64x64": (2, 2, 64, 64),  # the class absent in image 0 (with an ignore band) and filling image 1
}
TERM = {"term-2x3x19x65": (2, 3, 19, 65)}


def cases():
    return list(IMAGES) + list(VOLUMES) + list(MAPS) + list(TERM)


def seed_of(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def _blocks(rng, shape, side, high):
    """Integers below ``high`` in blocks of ``side`` pixels (distances of several pixels, not of one)"""
    small = rng.integers(0, high, tuple(shape[:-2]) + tuple(-(-s // side) for s in shape[-2:]))
    big = np.repeat(np.repeat(small, side, axis=-2), side, axis=-1)
    return big[..., :shape[-2], :shape[-1]]


def image_inputs(name):
    """sites, where (uint8), mask (uint8), target (int64), ignore of one image case"""
    B, H, W = IMAGES[name]
    rng = np.random.default_rng(seed_of(name))
    sites = (rng.random((B, H, W)) < 0.02).astype(np.uint8)
    where = (rng.random((B, H, W)) < 0.5).astype(np.uint8)
    mask = (rng.random((B, H, W)) < 0.03).astype(np.uint8)
    target = (rng.random((B, H, W)) < 0.03).astype(np.int64)
    ignore = -1
    if name == "img-3x40x65":
        target[0, :, 50:] = IGNORE
        target[2, 30:, :] = IGNORE
        ignore = IGNORE
    elif name == "img-1x1x4096":
        sites[:] = 0
        sites[0, 0, 0] = sites[0, 0, W - 1] = 1
        where = None
        mask = (rng.random((B, H, W)) < 0.5).astype(np.uint8)
        mask[0, 0, :8] = 0
        mask[0, 0, W - 1] = 1
        target[:] = 0
        target[0, 0, :3] = 1
    else:
        sites[1] = 0
        mask[1] = 0
        where = None
    return sites, where, mask, target, ignore


def _ties(shape):
    """Two volumes of 5 slices of 12 x 12: the prediction is the full first slice, the target the last
    slice without its last column.  The 2 * 12 * 11 distances between the two planes are equal (4 sz); the
    12 prediction voxels under the missing column are farther.  Volume 0: n = 276, ranks 261 and 262
    inside the run of 264 (no search for the next larger value).  Volume 1 (spacing 2.5, 0.75, 0.75) also
    loses two target voxels of its last kept column: n = 274, rank 259 is the run's last 100.0 and rank
    260 the first 100.5625 (the search runs).  Checked against the brute force of _boundary3d_ref.py."""
    N, H, W = shape
    mask = np.zeros(shape, np.uint8)
    target = np.zeros(shape, np.int64)
    mask[0] = 1
    target[4, :, :W - 1] = 1
    mask[5] = 1
    target[9, :, :W - 1] = 1
    target[9, :2, W - 2] = 0
    return mask, target


def volume_inputs(name):
    """sites, where, mask (uint8), target (int64), ignore of one volume case"""
    shape, depths, _ = VOLUMES[name]
    rng = np.random.default_rng(seed_of(name))
    dens = 0.3 if shape[0] > 1000 else 0.02
    sites = (rng.random(shape) < dens).astype(np.uint8)
    where = (rng.random(shape) < 0.5).astype(np.uint8)
    mask = (rng.random(shape) < dens).astype(np.uint8)
    target = (rng.random(shape) < dens).astype(np.int64)
    ignore = -1
    if name.startswith("vol-6x40x65"):
        mask[4:] = 0
        target[1, :, 60:] = IGNORE
        ignore = IGNORE
    elif name.endswith("ties"):
        mask, target = _ties(shape)
    return sites, where, mask, target, ignore


def map_inputs(name):
    """target (int64), ignore of one map case"""
    N, K, H, W = MAPS[name]
    rng = np.random.default_rng(seed_of(name))
    target = _blocks(rng, (N, H, W), 5, K).astype(np.int64)
    ignore = -100
    if name == "map-2x2x64x64":
        target[0] = 0
        target[0, :, 56:] = IGNORE
        target[1] = 1
        ignore = IGNORE
    elif name == "map-2x3x19x65":
        target[1, 15:, :] = IGNORE
        ignore = IGNORE
    return target, ignore


def term_inputs(name):
    """logits fp32 [N, K, H, W], target int64, phi fp32 [N, K-1, H, W], dlogits to add into, loss to add to"""
    N, K, H, W = TERM[name]
    rng = np.random.default_rng(seed_of(name))
    logits = (rng.standard_normal((N, K, H, W)) * 3.0).astype(np.float32)
    target = rng.integers(0, K, (N, H, W), dtype=np.int64)
    target[0, :, W - 9:] = IGNORE
    target[-1, H - 4:, :] = IGNORE
    phi = (rng.standard_normal((N, K - 1, H, W)) * 6.0).astype(np.float32)
    dl0 = rng.standard_normal((N, K, H, W)).astype(np.float32)
    return logits, target, phi, dl0, np.float32(0.375)


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def _filled(nbytes, dev):
    return torch.full((nbytes,), 0xAA, dtype=torch.uint8, device=dev)


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _image_digests(name, dev):
    from stfunet import _lib
    from stfunet._lib import call, stream
    B, H, W = IMAGES[name]
    sites, where, mask, target, ignore = (_dev(a, dev) if isinstance(a, np.ndarray) else a
                                          for a in image_inputs(name))
    nbytes = int(_lib.load().stf_boundary_scratch_bytes(B, H, W))
    out = {"scratch_bytes": nbytes}
    for key, wh in (("edt", None), ("edt_where", where)):
        if key == "edt_where" and wh is None:
            continue
        d2, scratch = _filled(B * H * W * 4, dev), _filled(nbytes, dev)
        call("stf_edt_sq", _ptr(sites), _ptr(wh), B, H, W, _ptr(d2), _ptr(scratch), stream())
        out[key] = _sha(d2)
    res, counts, scratch = _filled(B * 24, dev), _filled(B * 16, dev), _filled(nbytes, dev)
    call("stf_boundary_metrics", _ptr(mask), _ptr(target), B, H, W, ignore, _ptr(res), _ptr(counts), _ptr(scratch),
         stream())
    out["metrics"], out["counts"] = _sha(res), _sha(counts)
    out["metrics_value"] = [repr(v) for v in res.view(torch.float64).cpu().tolist()]
    return out


def _volume_digests(name, dev):
    from stfunet import _lib
    from stfunet._lib import call, stream
    (N, H, W), depths, spacing = VOLUMES[name]
    V = len(depths)
    sites, where, mask, target, ignore = (_dev(a, dev) if isinstance(a, np.ndarray) else a
                                          for a in volume_inputs(name))
    host = torch.zeros(V + 1, dtype=torch.int32)
    host[1:] = torch.tensor(depths).cumsum(0)
    starts, table = host.to(dev), torch.tensor(spacing, dtype=torch.float64).to(dev)
    nbytes = int(_lib.load().stf_boundary3d_scratch_bytes(N, H, W, V))
    out = {"scratch_bytes": nbytes}
    for key, wh in (("edt", None), ("edt_where", where)):
        d2, scratch = _filled(N * H * W * 8, dev), _filled(nbytes, dev)
        call("stf_edt3d_sq", _ptr(sites), _ptr(wh), N, H, W, _ptr(starts), host.data_ptr(), V, _ptr(table), _ptr(d2),
             _ptr(scratch), stream())
        out[key] = _sha(d2)
    res, counts, scratch = _filled(V * 24, dev), _filled(V * 16, dev), _filled(nbytes, dev)
    call("stf_boundary3d_metrics", _ptr(mask), _ptr(target), N, H, W, _ptr(starts), host.data_ptr(), V, _ptr(table),
         ignore, _ptr(res), _ptr(counts), _ptr(scratch), stream())
    out["metrics"], out["counts"] = _sha(res), _sha(counts)
    out["metrics_value"] = [repr(v) for v in res.view(torch.float64).cpu().tolist()]
    return out


def _map_digests(name, dev):
    from stfunet import _lib
    from stfunet._lib import call, stream
    N, K, H, W = MAPS[name]
    target, ignore = map_inputs(name)
    t = _dev(target, dev)
    nbytes = int(_lib.load().stf_sdf_scratch_bytes(N, H, W, K))
    phi, scratch = _filled(N * (K - 1) * H * W * 4, dev), _filled(nbytes, dev)
    call("stf_sdf", _ptr(t), N, H, W, K, ignore, _ptr(phi), _ptr(scratch), stream())
    return {"scratch_bytes": nbytes, "phi": _sha(phi)}


def _term_digests(name, dev):
    from stfunet import _lib
    from stfunet._lib import call, stream
    N, K, H, W = TERM[name]
    logits, target, phi, dl0, loss0 = term_inputs(name)
    x, t, p, dl = _dev(logits, dev), _dev(target, dev), _dev(phi, dev), _dev(dl0, dev)
    loss = torch.full((1,), float(loss0), device=dev)
    go = torch.full((1,), GRAD_OUT, device=dev)
    floats = int(_lib.load().stf_bloss_scratch_floats(N))
    part = _filled(floats * 4, dev).view(torch.float32)
    call("stf_bloss_fwd", _ptr(x), _ptr(t), _ptr(p), N, H, W, K, IGNORE, ALPHA, _ptr(part), _ptr(loss), stream())
    call("stf_bloss_bwd", _ptr(x), _ptr(t), _ptr(p), N, H, W, K, IGNORE, ALPHA, _ptr(go), _ptr(part[1:]), _ptr(dl),
         stream())
    return {"scratch_floats": floats, "partials": _sha(part), "loss": _sha(loss), "dlogits": _sha(dl),
            "loss_value": repr(float(loss[0]))}


def digests(name, dev="cuda"):
    fn = (_image_digests if name in IMAGES else _volume_digests if name in VOLUMES else
          _map_digests if name in MAPS else _term_digests)
    with torch.cuda.device(dev):
        out = fn(name, dev)
        torch.cuda.synchronize()
    return out
