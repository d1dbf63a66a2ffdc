"""A second, independent restatement of the voxel edits (include/vxrt.h, vxrt_edit_voxels; C: oracle/vxo_edit.c) in
numpy, on a bool [x, y, z] grid, written with slices and broadcasting so that the two restatements can be held against
each other.  TEST INFRASTRUCTURE ONLY (like the rest of oracle/): imported by tests/ alone."""
from __future__ import annotations

import numpy as np


def apply_edits(vox: np.ndarray, ops) -> np.ndarray:
    """Per op: the clipped box as a slice; a sphere as a mask of squared distances over it (|d| <= r < 2^31 inside the
    box: squares below 2^62, their sum in uint64).  Returns the edited copy; raises ValueError on an invalid op (all ops
    are checked before any change)."""
    out = np.array(vox, bool, copy=True)
    ops = [(o if isinstance(o, tuple) else (o.kind, o.value, tuple(o.a), tuple(o.b))) for o in ops]
    for kind, value, a, b in ops:
        if kind not in (0, 1) or value not in (0, 1) or (kind == 1 and (b[0] < 0 or b[1] != 0 or b[2] != 0)):
            raise ValueError("invalid edit op")
    for kind, value, a, b in ops:
        if kind == 0:
            lo, hi = [int(v) for v in a], [int(v) for v in b]
        else:
            lo, hi = [int(c) - int(b[0]) for c in a], [int(c) + int(b[0]) for c in a]
        lo = [max(l, 0) for l in lo]
        hi = [min(h, n - 1) for h, n in zip(hi, out.shape)]
        if any(l > h for l, h in zip(lo, hi)):
            continue
        box = tuple(slice(l, h + 1) for l, h in zip(lo, hi))
        if kind == 0:
            out[box] = bool(value)
            continue
        d = [(np.arange(l, h + 1, dtype=np.int64) - int(c)) for l, h, c in zip(lo, hi, a)]
        q = [(v * v).astype(np.uint64) for v in d]
        inside = (q[0][:, None, None] + q[1][None, :, None] + q[2][None, None, :]) <= np.uint64(int(b[0]) ** 2)
        out[box][inside] = bool(value)
    return out
