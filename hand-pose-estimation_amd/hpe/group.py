"""Lane groups (hpe_set_batch_groups): the numpy mirror of the group pick.

A group is a run of consecutive batch lanes that track one stream as independent subswarms
(lane seeds, hpe_set_batch_seeds).  After every tracked frame each group's rows {bestp[26], cost}
become the group's best row by hpe.dist.pick_best's rule -- the subswarm exchange's per-frame
best-of-N between lanes of one launch instead of ranks of a communicator:

  the smallest cost wins; a NaN cost never wins (NaN counts as +inf, +inf as the largest finite
  double, -inf as the lowest); ties go to the lowest lane; a group whose costs are all NaN takes
  its lowest lane's row.
"""
from __future__ import annotations

import numpy as np

STATE_LEN = 27  # bestp[26] + cost


def winners(rows, sizes):
    """The winning lane of every group: rows is (B, 27), sizes the groups' lane counts (positive,
    summing to B).  Returns one absolute lane index per group."""
    r = np.asarray(rows, dtype=np.float64)
    z = [int(v) for v in sizes]
    if r.ndim != 2 or r.shape[1] != STATE_LEN:
        raise ValueError("rows must be a (B, 27) array")
    if any(v < 1 for v in z) or sum(z) != r.shape[0]:
        raise ValueError(f"sizes {z} are not positive or do not sum to {r.shape[0]} lanes")
    out, at = [], 0
    for n in z:
        c = np.nan_to_num(r[at:at + n, STATE_LEN - 1], nan=np.inf)
        out.append(at + int(np.argmin(c)))  # the first minimum: the lowest lane
        at += n
    return out


def pick(rows, sizes):
    """rows with every group's rows replaced by the group's best row, bit for bit (a copy)."""
    r = np.array(rows, dtype=np.float64, copy=True)
    at = 0
    for n, w in zip(sizes, winners(r, sizes)):
        r[at:at + int(n)] = r[w].copy()
        at += int(n)
    return r
