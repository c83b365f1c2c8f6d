"""How the Gram-CTC golden vectors are stored: gram_ctc.npz holds every case, except that an array of more than SPLIT_BYTES
(the inputs and gradients of the |V| = 3000 cases) is kept one utterance per file, gram_ctc.<case>.<key>.<b>.npy, so that no
file passes 1 MiB.  Used by make_golden.py (to write them) and by the tests (to read them back as one table)."""
import os
import re

import numpy as np

SPLIT_BYTES = 512 << 10
_PART = re.compile(r"^gram_ctc\.(\w+\.\w+)\.(\d+)\.npy$")


def save(out_dir, arrays):
    small = {}
    for key, a in arrays.items():
        if a.nbytes > SPLIT_BYTES:
            for b in range(a.shape[1]):             # (T, B, V): axis 1 is the utterance
                np.save(os.path.join(out_dir, "gram_ctc.%s.%d.npy" % (key, b)), np.ascontiguousarray(a[:, b]))
        else:
            small[key] = a
    np.savez_compressed(os.path.join(out_dir, "gram_ctc.npz"), **small)


def load(golden_dir):
    with np.load(os.path.join(golden_dir, "gram_ctc.npz")) as z:
        table = {k: z[k] for k in z.files}
    parts = {}
    for name in os.listdir(golden_dir):
        m = _PART.match(name)
        if m:
            parts.setdefault(m.group(1), {})[int(m.group(2))] = np.load(os.path.join(golden_dir, name))
    for key, by_b in parts.items():
        assert key not in table and sorted(by_b) == list(range(len(by_b))), key
        table[key] = np.stack([by_b[b] for b in range(len(by_b))], axis=1)
    return table
