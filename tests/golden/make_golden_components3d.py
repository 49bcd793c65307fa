"""Generate tests/golden/components3d.npz: volumes and their connected-component labels by scipy.

    python tests/golden/make_golden_components3d.py

The expected values are ``scipy.ndimage.label(volume, generate_binary_structure(3, k))`` with k = 1, 2,
3 for connectivity 6, 18, 26: labels 1..n in raster order (z, y, x) of each component's first voxel,
and n.

Cases:
    rand_<D>x<H>x<W>_d<density>   seeded random volumes, 5x17x33 and 7x19x70, densities 0.05, 0.15
                                  (near the 26-neighbour percolation point), 0.3 (near the 6-neighbour
                                  one) and 0.5
    ball_specks                   one ball and scattered single voxels
    shell_core                    a hollow shell with a separate core inside
    tie                           two components of equal size in different slices (the raster-first
                                  one lies to the right)
    serpentine                    a 1-voxel-wide path that snakes through every slice, 5x9x66
    bridge                        two in-plane blobs that meet only through one voxel of the last slice
    space_diagonal                a corner-to-corner voxel chain: one component under 26, one per voxel
                                  under 6 and 18
    face_diagonal                 an edge-to-edge chain inside one row index: one component under 18
                                  and 26, one per voxel under 6
    checkerboard                  (z + y + x) even: one component under 18 and 26, one per voxel under 6
    single_slice                  depth 1: the 2-D labels
    empty, full                   no foreground, all foreground

Arrays, all cases in order: ``names``, ``shapes`` [n][3], ``mask`` (the cases' row-major bits packed per
case, ceil(D H W / 8) bytes, concatenated), ``n6`` / ``n18`` / ``n26`` [n] and ``labels6`` / ``labels18`` /
``labels26`` (uint16: the labels of each case's foreground voxels in raster order, concatenated).  The
archive is written with fixed timestamps, so a rerun reproduces it byte for byte.
"""
import io
import os
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DENSITIES = [0.05, 0.15, 0.3, 0.5]
CONNECTIVITIES = (6, 18, 26)


def cases():
    """[(name, uint8 volume)]."""
    rng = np.random.default_rng(20250301)
    out = []
    for D, H, W in ((5, 17, 33), (7, 19, 70)):
        for d in DENSITIES:
            out.append((f"rand_{D}x{H}x{W}_d{int(round(d * 1000)):03d}", (rng.random((D, H, W)) < d).astype(np.uint8)))
    zz, yy, xx = np.mgrid[0:12, 0:30, 0:70]
    m = ((zz - 6) ** 2 + (yy - 14) ** 2 + (xx - 40) ** 2 <= 5 ** 2).astype(np.uint8)
    for z, y, x in zip(rng.integers(0, 12, 30), rng.integers(0, 30, 30), rng.integers(0, 70, 30)):
        m[z, y, x] = 1
    out.append(("ball_specks", m))
    zz, yy, xx = np.mgrid[0:15, 0:21, 0:67]
    r2 = (zz - 7) ** 2 + (yy - 10) ** 2 + (xx - 33) ** 2
    out.append(("shell_core", (((r2 <= 7 ** 2) & (r2 >= 5 ** 2)) | (r2 <= 2 ** 2)).astype(np.uint8)))
    m = np.zeros((6, 12, 70), np.uint8)
    m[3:5, 2:5, 3:7] = 1                                        # 24 voxels, starts in slice 3
    m[1:3, 6:9, 62:66] = 1                                      # 24 voxels, starts in slice 1: raster-first
    out.append(("tie", m))
    m = np.zeros((5, 9, 66), np.uint8)
    for z in (0, 2, 4):                                         # every other row end to end, joined at
        m[z, ::2, :] = 1                                        # alternating ends: (0, 0) to (8, 65)
        for k, y in enumerate(range(1, 9, 2)):
            m[z, y, 65 if k % 2 == 0 else 0] = 1
    m[1, 8, 65] = m[3, 0, 0] = 1                                # the slices between join the paths' ends
    out.append(("serpentine", m))
    m = np.zeros((3, 20, 70), np.uint8)
    m[0:2, 2:8, 2:30] = 1
    m[0:2, 12:18, 40:68] = 1
    m[2, 7, 29:41] = 1
    m[2, 7:13, 40] = 1
    out.append(("bridge", m))
    m = np.zeros((8, 8, 70), np.uint8)
    for i in range(8):
        m[i, i, 60 + i] = 1
    out.append(("space_diagonal", m))
    m = np.zeros((8, 5, 70), np.uint8)
    for i in range(8):
        m[i, 2, 68 - i] = 1
    out.append(("face_diagonal", m))
    zz, yy, xx = np.mgrid[0:4, 0:6, 0:66]
    out.append(("checkerboard", ((zz + yy + xx) % 2 == 0).astype(np.uint8)))
    out.append(("single_slice", (rng.random((1, 23, 70)) < 0.45).astype(np.uint8)))
    out.append(("empty", np.zeros((3, 5, 70), np.uint8)))
    out.append(("full", np.ones((3, 5, 70), np.uint8)))
    return out


def scipy_label(volume, connectivity):
    from scipy.ndimage import generate_binary_structure, label
    labels, n = label(volume, generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity]))
    return labels.astype(np.int32), int(n)


def main():
    names, shapes, bits = [], [], []
    ns, labs = {c: [] for c in CONNECTIVITIES}, {c: [] for c in CONNECTIVITIES}
    for name, mask in cases():
        names.append(name)
        shapes.append(mask.shape)
        bits.append(np.packbits(mask.astype(bool).ravel()))
        for c in CONNECTIVITIES:
            labels, n = scipy_label(mask, c)
            assert n < 65536 and ((labels > 0) == (mask != 0)).all()
            ns[c].append(n)
            labs[c].append(labels[mask != 0].astype(np.uint16))
        print(f"{name:24s} {'x'.join(map(str, mask.shape)):10s} n6 {ns[6][-1]:5d} n18 {ns[18][-1]:5d} "
              f"n26 {ns[26][-1]:5d}")
    arrays = {"names": np.array(names), "shapes": np.array(shapes, np.int64), "mask": np.concatenate(bits)}
    for c in CONNECTIVITIES:
        arrays[f"n{c}"] = np.array(ns[c], np.int32)
        arrays[f"labels{c}"] = np.concatenate(labs[c])
    out = os.path.join(HERE, "components3d.npz")
    with zipfile.ZipFile(out, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.save(buf, arrays[k], allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                       compress_type=zipfile.ZIP_DEFLATED)
    print(f"wrote {out}: {len(names)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
