"""Fixture archives in parts: every committed file stays below 1 MiB, so make_golden.py / make_seam_fixture.py write `<base>_partN.npz`
(arrays in insertion order, a new part whenever the next array's deflated size would pass PART_BYTES).  The readers merge every part:
{name: array for part in sorted(glob(<base>_part*.npz)) ...}."""
import glob
import os
import zlib

import numpy as np

PART_BYTES = 900_000


def save_parts(base: str, arrays: dict) -> list:
    """base: path without the .npz suffix.  Removes the parts of an earlier run, writes the new ones, returns their paths."""
    for old in glob.glob(base + "_part*.npz"):
        os.remove(old)
    parts, cur, cur_bytes = [], {}, 0
    for name, a in arrays.items():
        n = len(zlib.compress(np.ascontiguousarray(a).tobytes(), 6))
        if cur and cur_bytes + n > PART_BYTES:
            parts.append(cur)
            cur, cur_bytes = {}, 0
        cur[name] = a
        cur_bytes += n
    if cur:
        parts.append(cur)
    paths = []
    for i, p in enumerate(parts):
        path = f"{base}_part{i}.npz"
        np.savez_compressed(path, **p)
        assert os.path.getsize(path) < 1 << 20, (path, os.path.getsize(path))
        paths.append(path)
    return paths
