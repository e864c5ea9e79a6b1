"""Host mirror of the lane views (hpe_batch_pipeline_begin_view, include/hpe.h "Lane views"): how
the 240x320 model image lies in a camera image, in plain numpy, for callers that reduce frames
themselves and for the tests.

Model pixel (r, c), 0 <= r < 240, 0 <= c < 320, reads camera pixel (sr, sc):
    sr = row0 + step * r
    sc = col0 + step * (319 - c if flags & FLIP_COLS else c)
and its value is cam[sr * pitch + sc] if 0 <= sr < height and 0 <= sc < width, else 0 -- a pick
(nearest-neighbour decimation): a hole at the picked pixel stays a hole.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

IMG_H, IMG_W = 240, 320
FLIP_COLS = 1          # HPE_VIEW_FLIP_COLS
DIM_MAX = 2048         # HPE_VIEW_DIM_MAX: pitch and height
PIXELS_MAX = 2097152   # HPE_VIEW_PIXELS_MAX: pitch * height
FIELDS = ("width", "height", "pitch", "row0", "col0", "step", "flags", "pad")


def _rint(x: float) -> int:
    """C's lrint under the default rounding mode: to nearest, ties to even."""
    return int(np.rint(np.float64(x)))


@dataclass(frozen=True)
class View:
    width: int
    height: int
    pitch: int
    row0: int
    col0: int
    step: int
    flags: int = 0
    pad: int = 0

    def __post_init__(self):
        for f in FIELDS:
            object.__setattr__(self, f, int(getattr(self, f)))

    @property
    def flip(self) -> bool:
        return bool(self.flags & FLIP_COLS)

    def check(self) -> "View":
        """The library's refusals (HPE_E_ARG there, ValueError here); returns self."""
        if not 1 <= self.step <= 8:
            raise ValueError(f"view step {self.step} outside 1..8")
        if self.width < 1 or self.height < 1 or self.pitch < self.width:
            raise ValueError(f"view of a {self.width} x {self.height} camera image with pitch "
                             f"{self.pitch}")
        if self.pitch > DIM_MAX or self.height > DIM_MAX or self.pitch * self.height > PIXELS_MAX:
            raise ValueError(f"view pitch {self.pitch} or height {self.height} above {DIM_MAX}, or "
                             f"more than {PIXELS_MAX} pixels per frame")
        if self.flags & ~FLIP_COLS or self.pad:
            raise ValueError(f"unknown view flags {self.flags:#x} or non-zero pad {self.pad}")
        return self

    @classmethod
    def fit(cls, width, height, pitch, fx, cx, cy, step, flags=0):
        """hpe_view_fit: (view, focal, residual_px) for a camera's intrinsics.  row0 =
        lrint(cy - 120 step), col0 = lrint(cx - 160 step) (159 under the flip), focal = fx / step;
        residual_px = the principal point's offset from model pixel (160, 120), {column, row},
        in model pixels: what the rounding left."""
        fx, cx, cy, step = float(fx), float(cx), float(cy), int(step)
        if not (np.isfinite(fx) and fx > 0 and np.isfinite(cx) and np.isfinite(cy)):
            raise ValueError("fx, cx, cy must be finite and fx positive")
        flip = bool(int(flags) & FLIP_COLS)
        if not (abs(cy - 120.0 * step) < 1e9 and abs(cx - (159.0 if flip else 160.0) * step) < 1e9):
            raise ValueError("the view's origin lies beyond +-1e9 pixels")
        v = cls(width, height, pitch, _rint(cy - 120.0 * step),
                _rint(cx - (159.0 if flip else 160.0) * step), step, flags).check()
        mc = (cx - v.col0) / step
        res = ((319.0 - mc if flip else mc) - 160.0, (cy - v.row0) / step - 120.0)
        return v, fx / step, res

    def camera_index(self):
        """(sr, sc, inside): for every model pixel the camera row and column it reads (int64,
        240x320 each) and whether that lies inside the camera image."""
        r = np.arange(IMG_H, dtype=np.int64)[:, None]
        c = np.arange(IMG_W, dtype=np.int64)[None, :]
        cc = (IMG_W - 1 - c) if self.flip else c
        sr = np.broadcast_to(self.row0 + self.step * r, (IMG_H, IMG_W))
        sc = np.broadcast_to(self.col0 + self.step * cc, (IMG_H, IMG_W))
        inside = (sr >= 0) & (sr < self.height) & (sc >= 0) & (sc < self.width)
        return sr, sc, inside

    def reduce(self, frame_u16):
        """The 240x320 uint16 model frame the view picks from a camera frame: a uint16 array of
        pitch * height pixels (flat, or (height, pitch)).  Nothing is converted silently."""
        f = np.asarray(frame_u16)
        if f.dtype != np.uint16:
            raise TypeError(f"View.reduce takes uint16 frames, got {f.dtype}")
        if f.size != self.pitch * self.height:
            raise ValueError(f"camera frame of {f.size} pixels, the view's is pitch * height = "
                             f"{self.pitch * self.height}")
        flat = f.reshape(-1)
        sr, sc, inside = self.camera_index()
        idx = np.clip(sr, 0, self.height - 1) * self.pitch + np.clip(sc, 0, self.width - 1)
        return np.where(inside, flat[idx], np.uint16(0)).astype(np.uint16)

    def to_camera(self, px):
        """Model pixels {column, row} (any shape (..., 2), fractional allowed: a report's px, a
        located centre) as camera pixels {column, row}."""
        p = np.asarray(px, dtype=np.float64)
        c, r = p[..., 0], p[..., 1]
        cc = (IMG_W - 1) - c if self.flip else c
        return np.stack([self.col0 + self.step * cc, self.row0 + self.step * r], axis=-1)

    def to_model(self, px):
        """Camera pixels {column, row} as model pixels {column, row}: to_camera's inverse."""
        p = np.asarray(px, dtype=np.float64)
        cc = (p[..., 0] - self.col0) / self.step
        r = (p[..., 1] - self.row0) / self.step
        return np.stack([(IMG_W - 1) - cc if self.flip else cc, r], axis=-1)


def as_view(v) -> View:
    """A View, an object with the eight fields (hpe._lib.View) or an 8-sequence (6: flags and
    pad 0) as a View."""
    if isinstance(v, View):
        return v
    if all(hasattr(v, f) for f in FIELDS):
        return View(*[getattr(v, f) for f in FIELDS])
    return View(*v)
