"""TEST INFRASTRUCTURE: a numpy restatement of the compact layers and the compose of include/sph_slab_probe.h.

The sums at the points are tests/probe_reference.py's, unchanged; this adds what a slab rank keeps of them -- the points its owned
particles touch, as (ascending indices, words) -- and the scatter-add that composes the ranks' layers.  Nothing here is imported by the
product."""
import numpy as np

from tests import probe_reference as pr


def layer(p, own, exps, PX, PY):
    """The layer of the rank that owns the particles `own` of `p` -> (uint32 indices ascending, int64[C+1, n_entries], footprints of the
    owned particles).  A touched point is an entry also where all of its words are 0."""
    raw, foot, touched = pr.raw_at_points(p.subset(own), exps, PX, PY)
    idx = np.flatnonzero(touched).astype(np.uint32)
    return idx, raw[:, touched], foot


def compose(planes, n_points, layers):
    """The scatter-add: layers = [(indices, words[planes, n_entries]) or None] -> (int64[planes, n_points], the points present in at
    least one layer)."""
    out = np.zeros((planes, n_points), np.int64)
    seen = np.zeros(n_points, bool)
    for l in layers:
        if l is None or len(l[0]) == 0:
            continue
        idx, words = np.asarray(l[0], np.int64), np.asarray(l[1], np.int64)
        assert words.shape == (planes, len(idx)) and (np.diff(idx) > 0).all() and (len(idx) == 0 or (idx[0] >= 0 and idx[-1] < n_points))
        out[:, idx] += words      # (the indices of one layer are distinct: a plain indexed add is the sum)
        seen[idx] = True
    return out, seen
