"""Generate tests/golden/components.npz: masks and their connected-component labels by scipy.

    python tests/golden/make_golden_components.py

The expected values are ``scipy.ndimage.label(mask, generate_binary_structure(2, 1))`` for
connectivity 4 and ``generate_binary_structure(2, 2)`` for connectivity 8: labels 1..n in raster order
of each component's first pixel, and n.

Cases:
    rand_<H>x<W>_d<density>   seeded random masks, 33x47 and 97x131, densities 0.2, 0.5, 0.593 (the
                              site-percolation threshold: the largest, most tortuous clusters), 0.8
    blob_specks               one disc and scattered single pixels and 2x2 specks
    ring_island               a ring with a separate island inside
    tie                       two components of equal area (the raster-first one lies to the right)
    u_shape, comb             arms that meet only in the last row: a late merge relabels whole arms
    spiral                    a 1-pixel-wide spiral at 64x64: the longest chains
    serpentine                a 1-pixel-wide path that runs every other row end to end
    diagonal, antidiagonal    pixel chains: one component under 8, one per pixel under 4
    checkerboard              64x64: 2048 components under 4, one under 8
    empty, full               no foreground, all foreground

Arrays, all cases in order: ``names``, ``shapes`` [n][2], ``mask`` (the cases' row-major bits packed
per case, ceil(H W / 8) bytes, concatenated), ``n4`` / ``n8`` [n] and ``labels4`` / ``labels8`` (uint16:
the labels of each case's foreground pixels in raster order, concatenated).  The archive is written
with fixed timestamps, so a rerun reproduces it byte for byte.
"""
import io
import os
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DENSITIES = [0.2, 0.5, 0.593, 0.8]


def spiral(n):
    """A 1-pixel-wide square spiral with 1-pixel gaps, wound inward from the top-left corner."""
    m = np.zeros((n, n), np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = 1
    while True:
        moved = False
        for _ in range(4):
            steps = 0
            while True:
                ny, nx = y + dy, x + dx
                ay, ax = ny + dy, nx + dx                      # the pixel after the next must stay clear
                if not (0 <= ny < n and 0 <= nx < n) or m[ny, nx]:
                    break
                if 0 <= ay < n and 0 <= ax < n and m[ay, ax]:
                    break
                y, x = ny, nx
                m[y, x] = 1
                steps += 1
            moved |= steps > 1
            dy, dx = dx, -dy                                   # turn right
        if not moved:
            return m


def cases():
    """[(name, uint8 mask)]."""
    rng = np.random.default_rng(20241020)
    out = []
    for H, W in ((33, 47), (97, 131)):
        for d in DENSITIES:
            out.append((f"rand_{H}x{W}_d{int(round(d * 1000)):03d}", (rng.random((H, W)) < d).astype(np.uint8)))
    yy, xx = np.mgrid[0:70, 0:90]
    m = ((yy - 30) ** 2 + (xx - 40) ** 2 <= 15 ** 2).astype(np.uint8)
    for y, x in zip(rng.integers(0, 69, 25), rng.integers(0, 89, 25)):
        m[y, x] = 1
        if (y + x) % 3 == 0:
            m[y:y + 2, x:x + 2] = 1
    out.append(("blob_specks", m))
    yy, xx = np.mgrid[0:41, 0:67]
    r2 = (yy - 20) ** 2 + (xx - 33) ** 2
    out.append(("ring_island", (((r2 <= 18 ** 2) & (r2 >= 14 ** 2)) | (r2 <= 5 ** 2)).astype(np.uint8)))
    m = np.zeros((20, 70), np.uint8)
    m[8:12, 3:9] = 1                                            # 24 pixels, starts in row 8
    m[5:11, 60:64] = 1                                          # 24 pixels, starts in row 5: raster-first
    out.append(("tie", m))
    m = np.zeros((40, 70), np.uint8)
    m[:, 2] = m[:, 67] = 1
    m[39, 2:68] = 1
    out.append(("u_shape", m))
    m = np.zeros((30, 131), np.uint8)
    m[:, ::2] = 1
    m[29, :] = 1
    out.append(("comb", m))
    out.append(("spiral", spiral(64)))
    m = np.zeros((21, 66), np.uint8)
    m[::2, :] = 1
    for k, y in enumerate(range(1, 21, 2)):
        m[y, 65 if k % 2 == 0 else 0] = 1
    out.append(("serpentine", m))
    out.append(("diagonal", np.eye(50, 70, dtype=np.uint8)))
    out.append(("antidiagonal", np.eye(50, 70, dtype=np.uint8)[:, ::-1].copy()))
    yy, xx = np.mgrid[0:64, 0:64]
    out.append(("checkerboard", ((yy + xx) % 2 == 0).astype(np.uint8)))
    out.append(("empty", np.zeros((9, 70), np.uint8)))
    out.append(("full", np.ones((9, 70), np.uint8)))
    return out


def scipy_label(mask, connectivity):
    from scipy.ndimage import generate_binary_structure, label
    labels, n = label(mask, generate_binary_structure(2, 1 if connectivity == 4 else 2))
    return labels.astype(np.int32), int(n)


def main():
    names, shapes, bits = [], [], []
    ns, labs = {4: [], 8: []}, {4: [], 8: []}
    for name, mask in cases():
        names.append(name)
        shapes.append(mask.shape)
        bits.append(np.packbits(mask.astype(bool).ravel()))
        for c in (4, 8):
            labels, n = scipy_label(mask, c)
            assert n < 65536 and ((labels > 0) == (mask != 0)).all()
            ns[c].append(n)
            labs[c].append(labels[mask != 0].astype(np.uint16))
        print(f"{name:24s} {mask.shape[0]:3d}x{mask.shape[1]:<3d} n4 {ns[4][-1]:5d} n8 {ns[8][-1]:5d}")
    arrays = {"names": np.array(names), "shapes": np.array(shapes, np.int64), "mask": np.concatenate(bits)}
    for c in (4, 8):
        arrays[f"n{c}"] = np.array(ns[c], np.int32)
        arrays[f"labels{c}"] = np.concatenate(labs[c])
    out = os.path.join(HERE, "components.npz")
    with zipfile.ZipFile(out, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.save(buf, arrays[k], allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                       compress_type=zipfile.ZIP_DEFLATED)
    print(f"wrote {out}: {len(names)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
