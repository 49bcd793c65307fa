"""Generate tests/golden/boundary3d.npz: seeded blob volumes and their per-case boundary metrics by scipy.

    python tests/golden/make_golden_boundary3d.py

The expected values are MedPy's hd / hd95 / assd (medpy/metric/binary.py, ``__surface_distances``)
on a 3-D array with ``voxelspacing=(sz, sy, sx)`` and ``connectivity=1``, restated on scipy and
numpy the way MedPy computes them:

    border   M ^ binary_erosion(M, generate_binary_structure(3, 1))         (border_value=0)
    dt       distance_transform_edt(~border_of_the_other_mask, sampling=(sz, sy, sx))
    sds      dt[border]                                  both directions
    hd       max(sds_pt.max(), sds_tp.max())
    hd95     np.percentile(np.hstack((sds_pt, sds_tp)), 95)
    assd     np.mean((sds_pt.mean(), sds_tp.mean()))

with NaN x3 where MedPy raises (an empty mask on either side).

Cases: volumes of 1x40x66, 2x33x65, 5x20x70, 12x24x40 and 4x37x130 voxels, each with a few
lesion-sized ellipsoid blobs as T and P = other blobs around the same centres (``<shape>_blobs``),
once with P = T shifted by one voxel along every axis (``..._shift``: small distances) and, for the
first and the last shape, with an empty P (``..._empty``).  ``spacings`` [2][3] holds the two voxel
spacings, (1, 1, 1) and (2.5, 0.75, 0.75); ``metrics`` [n][2][3] = (hd, hd95, assd) float64 at each;
``names``, ``shapes`` [n][3]; and ``P``, ``T``, ``border_p``, ``border_t``, each the cases' row-major
bits packed per case (ceil(D H W / 8) bytes) and concatenated.  The archive is written with fixed
timestamps, so a rerun reproduces it byte for byte.
"""
import io
import os
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(1, 40, 66), (2, 33, 65), (5, 20, 70), (12, 24, 40), (4, 37, 130)]
SPACINGS = [(1.0, 1.0, 1.0), (2.5, 0.75, 0.75)]


def scipy_border(m):
    from scipy.ndimage import binary_erosion, generate_binary_structure
    m = np.asarray(m).astype(bool)
    return m ^ binary_erosion(m, generate_binary_structure(3, 1))


def scipy_metrics(P, T, spacing):
    """(border_p, border_t, hd, hd95, assd) of one volume as MedPy computes them."""
    from scipy.ndimage import distance_transform_edt
    bp, bt = scipy_border(P), scipy_border(T)
    nan = float("nan")
    if not bp.any() or not bt.any():
        return bp, bt, nan, nan, nan
    pt = distance_transform_edt(~bt, sampling=spacing)[bp]
    tp = distance_transform_edt(~bp, sampling=spacing)[bt]
    return (bp, bt, float(max(pt.max(), tp.max())), float(np.percentile(np.hstack((pt, tp)), 95)),
            float(np.mean((pt.mean(), tp.mean()))))


def blobs(rng, shape, centres, scale):
    """uint8 [D, H, W]: the union of one ellipsoid per centre with seeded radii."""
    D, H, W = shape
    Z, Y, X = np.mgrid[0:D, 0:H, 0:W]
    out = np.zeros(shape, bool)
    for cz, cy, cx in centres:
        rz, ry, rx = rng.uniform(0.6, 2.5), rng.uniform(2.0, 5.0) * scale, rng.uniform(2.0, 6.0) * scale
        out |= ((Z - cz) / rz) ** 2 + ((Y - cy) / ry) ** 2 + ((X - cx) / rx) ** 2 <= 1.0
    return out.astype(np.uint8)


def shift1(m):
    out = np.zeros_like(m)
    D = m.shape[0]
    if D > 1:
        out[1:, 1:, 1:] = m[:-1, :-1, :-1]
    else:
        out[:, 1:, 1:] = m[:, :-1, :-1]
    return out


def random_cases():
    """[(name, P, T)] with uint8 masks, from one seeded generator."""
    rng = np.random.default_rng(20240923)
    cases = []
    for shape in SHAPES:
        D, H, W = shape
        centres = [(rng.uniform(0, D - 1), rng.uniform(4, H - 5), rng.uniform(5, W - 6)) for _ in range(3)]
        T = blobs(rng, shape, centres, 1.0)
        moved = [(cz + rng.uniform(-0.7, 0.7), cy + rng.uniform(-2, 2), cx + rng.uniform(-3, 3)) for cz, cy, cx in centres]
        P = blobs(rng, shape, moved[:2] + [(rng.uniform(0, D - 1), rng.uniform(4, H - 5), rng.uniform(5, W - 6))], 0.9)
        name = "x".join(str(s) for s in shape)
        cases.append((name + "_blobs", P, T))
        cases.append((name + "_shift", shift1(T), T))
        if shape in (SHAPES[0], SHAPES[-1]):
            cases.append((name + "_empty", np.zeros_like(T), T))
    return cases


def main():
    names, shapes, values = [], [], []
    bits = {k: [] for k in ("P", "T", "border_p", "border_t")}
    for name, P, T in random_cases():
        rows = []
        for sp in SPACINGS:
            bp, bt, hd, hd95, assd = scipy_metrics(P, T, sp)
            rows.append((hd, hd95, assd))
        names.append(name)
        shapes.append(P.shape)
        values.append(rows)
        for k, v in (("P", P), ("T", T), ("border_p", bp), ("border_t", bt)):
            bits[k].append(np.packbits(np.asarray(v).astype(bool).ravel()))
        print(name, int(bp.sum()), int(bt.sum()), rows)
    arrays = {k: np.concatenate(v) for k, v in bits.items()}
    arrays["names"] = np.array(names)
    arrays["shapes"] = np.array(shapes, np.int64)
    arrays["metrics"] = np.array(values, np.float64)
    arrays["spacings"] = np.array(SPACINGS, np.float64)
    out = os.path.join(HERE, "boundary3d.npz")
    with zipfile.ZipFile(out, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.save(buf, arrays[k], allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                       compress_type=zipfile.ZIP_DEFLATED)
    defined = int((~np.isnan(arrays["metrics"][:, 0, 0])).sum())
    print(f"wrote {out}: {len(names)} cases ({defined} defined), {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
