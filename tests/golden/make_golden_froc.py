"""Writes tests/golden/froc.npz: the inputs and the expected summary, table and confidence histogram of
every case of tests/_froc_ref.py ``cases()``.

The labels come from ``scipy.ndimage.label`` (scipy was importable where this fixture was made), not
from the numpy labeller the restatement uses: the definition's arithmetic is shared, the labelling is
independent.  Masks and targets are stored as uint8, scores as float32.

    python tests/golden/make_golden_froc.py
"""
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from _components3d_ref import LEVEL  # noqa: E402
from _froc_ref import cases, run_case  # noqa: E402


def scipy_label(volume, connectivity):
    labels, n = ndimage.label(volume, ndimage.generate_binary_structure(3, LEVEL[connectivity]))
    return labels.astype(np.int32), int(n)


def main():
    out, names = {}, []
    for c in cases():
        name = c["name"]
        names.append(name)
        assert c["target"].min() >= 0 and c["target"].max() <= 255
        out[name + "/mask"], out[name + "/scores"] = c["mask"], c["scores"]
        out[name + "/target"], out[name + "/depths"] = c["target"].astype(np.uint8), np.array(c["depths"], np.int64)
        out[name + "/params"] = np.array([c["bins"], c["connectivity"], c["max_lesions"],
                                          -1 if c["ignore"] is None else c["ignore"]], np.int64)
        out[name + "/min_overlap"] = np.float64(c["min_overlap"])
        out[name + "/summary"], out[name + "/table"], out[name + "/hist"] = run_case(c, scipy_label)
    path = os.path.join(HERE, "froc.npz")
    np.savez_compressed(path, names=np.array(names), **out)
    print(path, os.path.getsize(path), "bytes,", len(names), "cases")


if __name__ == "__main__":
    main()
