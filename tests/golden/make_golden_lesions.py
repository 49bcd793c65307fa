"""Writes tests/golden/lesions.npz: the expected summary and lesion table of every case of
tests/_lesion_ref.py ``cases()``.

The labels come from ``scipy.ndimage.label`` (scipy was importable where this fixture was made), not
from the numpy labeller the restatement uses: the definition's arithmetic is shared, the labelling is
independent.  Inputs are not stored; ``cases()`` rebuilds them (seeded PCG64 and literals).

    python tests/golden/make_golden_lesions.py
"""
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from _components3d_ref import LEVEL  # noqa: E402
from _lesion_ref import cases, stack_metrics  # noqa: E402


def scipy_label(volume, connectivity):
    labels, n = ndimage.label(volume, ndimage.generate_binary_structure(3, LEVEL[connectivity]))
    return labels.astype(np.int32), int(n)


def main():
    out, names = {}, []
    for c in cases():
        summary, table = stack_metrics(c["mask"], c["target"], c["depths"], c["connectivity"], c["min_overlap"],
                                       c["max_lesions"], c["ignore"], labeller=scipy_label)
        names.append(c["name"])
        out[c["name"] + "/summary"], out[c["name"] + "/table"] = summary, table
    path = os.path.join(HERE, "lesions.npz")
    np.savez_compressed(path, names=np.array(names), **out)
    print(path, os.path.getsize(path), "bytes,", len(names), "cases")


if __name__ == "__main__":
    main()
