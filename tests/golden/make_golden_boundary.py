"""Generate tests/golden/boundary.npz: seeded random mask pairs and their boundary metrics by scipy.

    python tests/golden/make_golden_boundary.py

The expected values are MedPy's hd / hd95 / assd (medpy/metric/binary.py, ``__surface_distances``)
restated on scipy and numpy, the way MedPy computes them:

    border   M ^ binary_erosion(M, generate_binary_structure(2, 1))         (border_value=0)
    dt       distance_transform_edt(~border_of_the_other_mask)
    sds      dt[border]                                  both directions
    hd       max(sds_pt.max(), sds_tp.max())
    hd95     np.percentile(np.hstack((sds_pt, sds_tp)), 95)
    assd     np.mean((sds_pt.mean(), sds_tp.mean()))

with NaN x3 where MedPy raises (an empty mask on either side).

Cases: shapes 1x1, 1x7, 9x1, 5x5, 33x65, 37x130 at densities 0.02, 0.3, 0.7, 0.98, each once with
independent P and T (``<shape>_d<density>``) and once with P a dilation of T by the 3x3 square
(``..._dil``: overlapping masks, small distances).  Seven arrays hold all cases in order: ``names``,
``shapes`` [n][2], ``metrics`` [n][3] = (hd, hd95, assd) float64, and ``P``, ``T``, ``border_p``,
``border_t``, each the cases' row-major bits packed per case (ceil(H W / 8) bytes) and concatenated.
The archive is written with fixed timestamps, so a rerun reproduces it byte for byte.
"""
import io
import os
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(1, 1), (1, 7), (9, 1), (5, 5), (33, 65), (37, 130)]
DENSITIES = [0.02, 0.3, 0.7, 0.98]


def scipy_border(m):
    from scipy.ndimage import binary_erosion, generate_binary_structure
    m = np.asarray(m).astype(bool)
    return m ^ binary_erosion(m, generate_binary_structure(2, 1))


def scipy_metrics(P, T):
    """(border_p, border_t, hd, hd95, assd) of one image as MedPy computes them."""
    from scipy.ndimage import distance_transform_edt
    bp, bt = scipy_border(P), scipy_border(T)
    nan = float("nan")
    if not bp.any() or not bt.any():
        return bp, bt, nan, nan, nan
    pt = distance_transform_edt(~bt)[bp]
    tp = distance_transform_edt(~bp)[bt]
    return (bp, bt, float(max(pt.max(), tp.max())), float(np.percentile(np.hstack((pt, tp)), 95)),
            float(np.mean((pt.mean(), tp.mean()))))


def dilate3(m):
    q = np.pad(m.astype(bool), 1)
    out = np.zeros_like(m, dtype=bool)
    for dy in range(3):
        for dx in range(3):
            out |= q[dy:dy + m.shape[0], dx:dx + m.shape[1]]
    return out


def random_cases():
    """[(name, P, T)] with uint8 masks, from one seeded generator."""
    rng = np.random.default_rng(20240611)
    cases = []
    for H, W in SHAPES:
        for d in DENSITIES:
            T = rng.random((H, W)) < d
            P = rng.random((H, W)) < d
            name = f"{H}x{W}_d{int(round(d * 100)):02d}"
            cases.append((name, P.astype(np.uint8), T.astype(np.uint8)))
            cases.append((name + "_dil", dilate3(T).astype(np.uint8), T.astype(np.uint8)))
    return cases


def main():
    names, shapes, values = [], [], []
    bits = {k: [] for k in ("P", "T", "border_p", "border_t")}
    for name, P, T in random_cases():
        bp, bt, hd, hd95, assd = scipy_metrics(P, T)
        names.append(name)
        shapes.append(P.shape)
        values.append((hd, hd95, assd))
        for k, v in (("P", P), ("T", T), ("border_p", bp), ("border_t", bt)):
            bits[k].append(np.packbits(np.asarray(v).astype(bool).ravel()))
    arrays = {k: np.concatenate(v) for k, v in bits.items()}
    arrays["names"] = np.array(names)
    arrays["shapes"] = np.array(shapes, np.int64)
    arrays["metrics"] = np.array(values, np.float64)
    out = os.path.join(HERE, "boundary.npz")
    with zipfile.ZipFile(out, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.save(buf, arrays[k], allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                       compress_type=zipfile.ZIP_DEFLATED)
    defined = int((~np.isnan(arrays["metrics"][:, 0])).sum())
    print(f"wrote {out}: {len(names)} cases ({defined} defined), {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
