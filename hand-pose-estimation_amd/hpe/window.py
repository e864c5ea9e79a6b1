"""Host mirror of the lane windows (hpe_set_batch_window, include/hpe.h): the masking rule and
the pose rule in plain numpy, for callers that mask frames themselves and for the tests.

A window is (row_lo, row_hi, col_lo, col_hi, z_lo, z_hi), every bound inclusive: rows 0..239,
columns 0..319, depth in the converted unit (cm with to_cm).  `Window` is a named tuple; every
function here takes any 6-sequence or an object with those attributes (hpe._lib.Window).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

IMG_H, IMG_W = 240, 320
FIELDS = ("row_lo", "row_hi", "col_lo", "col_hi", "z_lo", "z_hi")
Window = namedtuple("Window", FIELDS)
WHOLE = Window(0, IMG_H - 1, 0, IMG_W - 1, -np.inf, np.inf)
EMPTY = Window(1, 0, 1, 0, 1.0, 0.0)


def as_window(win) -> Window:
    """Any 6-sequence, or an object with the six fields, as a Window (ints and floats)."""
    if all(hasattr(win, f) for f in FIELDS):
        v = [getattr(win, f) for f in FIELDS]
    else:
        v = list(win)
        if len(v) != 6:
            raise ValueError("a window is (row_lo, row_hi, col_lo, col_hi, z_lo, z_hi)")
    return Window(int(v[0]), int(v[1]), int(v[2]), int(v[3]), float(v[4]), float(v[5]))


def keep_mask(depth_mm, win, to_cm=True):
    """The masking rule: pixel (r, c) with raw value rv is kept iff row_lo <= r <= row_hi,
    col_lo <= c <= col_hi and z_lo <= Z <= z_hi, Z = rv / 10 in fp64 with to_cm, else rv."""
    w = as_window(win)
    d = np.asarray(depth_mm, dtype=np.float32).reshape(IMG_H, IMG_W)
    Z = d.astype(np.float64) / 10. if to_cm else d.astype(np.float64)
    r = np.arange(IMG_H)[:, None]
    c = np.arange(IMG_W)[None, :]
    with np.errstate(invalid="ignore"):
        return ((r >= w.row_lo) & (r <= w.row_hi) & (c >= w.col_lo) & (c <= w.col_hi) &
                (Z >= w.z_lo) & (Z <= w.z_hi))


def apply(depth_mm, win, to_cm=True):
    """The frame as the windowed preparation reads it: every pixel the window does not keep
    is 0.0f.  Returns a new float32 (240, 320) array."""
    d = np.asarray(depth_mm, dtype=np.float32).reshape(IMG_H, IMG_W)
    return np.where(keep_mask(d, win, to_cm), d, np.float32(0.0)).astype(np.float32)


def from_spheres(S, radii, focal, margin_xy, margin_z) -> Window:
    """The pose rule on the 48 centres S of hpe_build_spheres (y and z negated, as it returns
    them) and the hand's radii.  Every product is rounded before its add (plain fp64 numpy)."""
    S = np.asarray(S, dtype=np.float64).reshape(-1, 3)
    R = np.asarray(radii, dtype=np.float64).ravel()
    focal, mxy, mz = np.float64(focal), np.float64(margin_xy), np.float64(margin_z)
    x = S[:, 0]
    y = S[:, 1] * -1
    z = S[:, 2] * -1
    if not (np.isfinite(x).all() and np.isfinite(y).all() and np.isfinite(z).all()) or (z <= 0).any():
        return WHOLE  # fail open: a NaN pose, a hand at or behind the camera
    with np.errstate(over="ignore", invalid="ignore"):
        e = R + mxy
        cl = np.floor((focal * (x - e) + 160.0 * z) / z)
        ch = np.floor((focal * (x + e) + 160.0 * z) / z)
        rl = np.floor((focal * (y - e) + 120.0 * z) / z)
        rh = np.floor((focal * (y + e) + 120.0 * z) / z)
        zl = z - (R + mz)
        zh = z + (R + mz)
    return Window(int(min(max(rl.min(), 0.0), 240.0)), int(min(max(rh.max(), -1.0), 239.0)),
                  int(min(max(cl.min(), 0.0), 320.0)), int(min(max(ch.max(), -1.0), 319.0)),
                  float(zl.min()), float(zh.max()))


def is_whole(win) -> bool:
    w = as_window(win)
    return (w.row_lo <= 0 and w.row_hi >= IMG_H - 1 and w.col_lo <= 0 and w.col_hi >= IMG_W - 1 and
            w.z_lo == -np.inf and w.z_hi == np.inf)
