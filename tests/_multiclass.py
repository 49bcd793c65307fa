"""The reference-generated many-class criterion cases (tests/golden/multiclass.npz, written by
tests/golden/make_golden_multiclass.py) as the dicts ``_criterion_ref.fixture_entries`` returns."""
import os

import numpy as np
import torch

from _criterion_ref import GOLDEN


def _entries():
    g = np.load(os.path.join(GOLDEN, "multiclass.npz"))
    out = []
    for name in g["names"].tolist():
        w = g[name + ".weight"]
        case = str(g[name + ".case"])
        out.append(dict(name=name, logits=torch.from_numpy(g[case + ".logits"]),
                        target=torch.from_numpy(g[case + ".target"]),
                        weight=torch.from_numpy(w) if w.size else None,
                        ignore_index=int(g[name + ".ignore_index"]), dice=bool(g[name + ".dice"]),
                        loss=float(g[name + ".loss"]), grad=torch.from_numpy(g[name + ".grad"])))
    return out


MC_ENTRIES = _entries()
