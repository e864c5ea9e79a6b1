"""Lane reports (hpe_set_batch_report): the host mirror of the report's pixel rule and a numpy
view of one report.

project_joints is what k_report_b and k_lane_joints_b compute per joint, in numpy fp64 with the
same operations in the same order (numpy never fuses a product into an add):
    column = (focal x + 160 z) / z,   row = (focal y + 120 z) / z
on the joint's camera coordinates (hand_joints is not negated), both NaN when a coordinate is not
finite or z <= 0.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import _lib

Report = namedtuple("Report", "seq call lane kind n flags bad_streak state joints px")


def project_joints(joints, focal=241.42):
    """{column, row} of every joint in the 320x240 image: (..., 3) -> (..., 2), fp64."""
    j = np.asarray(joints, dtype=np.float64)
    if j.shape[-1] != 3:
        raise ValueError(f"joints of shape {j.shape}: the last axis holds x, y, z")
    focal = np.float64(focal)
    x, y, z = j[..., 0], j[..., 1], j[..., 2]
    with np.errstate(all="ignore"):
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (z > 0)
        col = (focal * x + np.float64(160.0) * z) / z
        row = (focal * y + np.float64(120.0) * z) / z
    out = np.empty(j.shape[:-1] + (2,), dtype=np.float64)
    out[..., 0] = np.where(ok, col, np.nan)
    out[..., 1] = np.where(ok, row, np.nan)
    return out


def as_report(r: _lib.LaneReport) -> Report:
    """A hpe_lane_report as numpy copies: state (27,), joints (21, 3), px (21, 2)."""
    return Report(int(r.seq), int(r.call), int(r.lane), int(r.kind), int(r.n), int(r.flags),
                  int(r.bad_streak), np.array(r.state, dtype=np.float64),
                  np.array(r.joints, dtype=np.float64).reshape(21, 3),
                  np.array(r.px, dtype=np.float64).reshape(21, 2))
